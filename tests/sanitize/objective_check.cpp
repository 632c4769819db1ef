// objective_check.cpp — the workspace layout of the fused training objective (csrc/host_plan.hpp objective_layout;
// dad_train_objective_forward / dad_train_objective_backward), walked on the host without HIP under
// -fsanitize=address,undefined against what the kernels of csrc/train_objective.hpp assume:
//   * the new regions of `saved` and `scratch` start behind the existing parts, at multiples of 16 bytes, hold what
//     the kernels write into them, do not overlap, and end at the sizes dad_train_objective_workspace_bytes reports;
//   * the existing sizes (dad_train_workspace_bytes) are untouched;
//   * the K slices of d act = d rows . W cover temb_width exactly once in whole 128-column steps (32 per wave), and a
//     32-column chunk never straddles two ResidualTemporalBlocks;
//   * the time gradient list names every time-MLP tensor once, at aligned offsets, with the element counts of the
//     expected shapes.
// Built and run by tests/test_objective_host.py (CPU suite).
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../dynamics_aware_diffusion_amd/csrc/host_plan.hpp"

using namespace dadhost;

static int g_failures = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            ++g_failures;                                                                 \
            fprintf(stderr, "CHECK failed %s:%d: %s — ", __FILE__, __LINE__, #cond);      \
            fprintf(stderr, __VA_ARGS__);                                                 \
            fprintf(stderr, "\n");                                                        \
        }                                                                                 \
    } while (0)

struct Arch {
    const char* name;
    int td, dim, time_dim, horizon;
    std::vector<int> mults;
    std::vector<int> real;        // dad_model_set_group_channels (empty: unpadded)
    int hreal;                    // dad_model_set_horizon (0: unpadded)
};

struct Region { const char* name; long at, floats; };

// regions in floats from the start of the new part: aligned, inside [0, total), pairwise disjoint; every float of the
// part is touched through a byte map the sanitizer watches
static void check_regions(const char* arch, int B, const char* what, const std::vector<Region>& rs, long total) {
    std::vector<unsigned char> owner((size_t)total, 0);
    int id = 0;
    for (const Region& r : rs) {
        ++id;
        CHECK(r.at >= 0 && r.floats > 0 && r.at + r.floats <= total, "%s B=%d %s.%s: [%ld, %ld) of %ld", arch, B, what, r.name, r.at,
              r.at + r.floats, total);
        CHECK((r.at * (long)sizeof(float)) % 16 == 0, "%s B=%d %s.%s: offset %ld floats is not 16-byte aligned", arch, B, what, r.name, r.at);
        if (r.at < 0 || r.at + r.floats > total) continue;
        for (long i = r.at; i < r.at + r.floats; ++i) {
            CHECK(owner[(size_t)i] == 0, "%s B=%d %s.%s overlaps region %d at float %ld", arch, B, what, r.name, (int)owner[(size_t)i], i);
            if (owner[(size_t)i] != 0) break;
            owner[(size_t)i] = (unsigned char)id;
        }
    }
}

static void check_arch(const Arch& a) {
    HostModel m;
    dad_cfg& c = m.cfg;
    c.transition_dim = a.td; c.dim = a.dim; c.time_dim = a.time_dim;
    c.n_levels = (int)a.mults.size();
    for (size_t i = 0; i < a.mults.size(); ++i) c.channels[i] = a.dim * a.mults[i];
    c.kernel_size = 5; c.horizon = a.horizon; c.n_timesteps = 20;
    c.predict_epsilon = c.clip_denoised = 1;
    int rc = check_cfg(&c);
    CHECK(rc == DAD_OK, "%s: check_cfg: %s", a.name, g_err);
    if (rc != DAD_OK) return;
    for (size_t i = 0; i < a.real.size(); ++i) m.real_channels[i] = a.real[i];
    m.real_horizon = a.hreal;
    m.training = true;
    rc = build_plan(&m);
    CHECK(rc == DAD_OK, "%s: build_plan: %s", a.name, g_err);
    if (rc != DAD_OK) return;

    // the time gradient list against the expected shapes
    const long tdm = c.time_dim;
    const int W = m.tplan.temb_width;
    const std::vector<TimeBlockRef> blocks = time_block_list(m);
    CHECK(blocks.size() == 4 * a.mults.size() && blocks.size() <= (size_t)4 * DAD_MAX_LEVELS, "%s: %zu blocks", a.name, blocks.size());
    int next = 0;
    for (const TimeBlockRef& b : blocks) {
        CHECK(b.off == next && b.off % 32 == 0 && b.cout % 32 == 0, "%s: block %s at %d (+%d), expected %d", a.name, b.base.c_str(), b.off, b.cout, next);
        next = b.off + b.cout;
    }
    CHECK(next == W, "%s: blocks end at %d, temb_width %d", a.name, next, W);
    CHECK(m.time_grad_slots.size() == 4 + 2 * blocks.size(), "%s: %zu time gradient slots", a.name, m.time_grad_slots.size());
    std::set<std::string> seen;
    long end = 0, time_keys = 0;
    for (const auto& kv : m.expected) time_keys += kv.first.find("time_mlp.") != std::string::npos;
    for (const HostModel::GradSlot& s : m.time_grad_slots) {
        CHECK(seen.insert(s.key).second, "%s: %s listed twice", a.name, s.key.c_str());
        const auto it = m.expected.find(s.key);
        CHECK(it != m.expected.end(), "%s: %s is not a parameter", a.name, s.key.c_str());
        if (it == m.expected.end()) continue;
        long n = 1;
        for (int64_t d : it->second) n *= (long)d;
        CHECK(n == s.numel, "%s: %s has %ld elements, the slot %ld", a.name, s.key.c_str(), n, s.numel);
        CHECK(s.offset >= end && s.offset % 4 == 0, "%s: %s at %ld behind %ld", a.name, s.key.c_str(), s.offset, end);
        end = s.offset + s.numel;
    }
    CHECK((long)seen.size() == time_keys, "%s: %zu of %ld time-MLP tensors listed", a.name, seen.size(), time_keys);
    CHECK(end <= m.time_grad_numel, "%s: slots end at %ld of %ld", a.name, end, m.time_grad_numel);
    for (const HostModel::GradSlot& s : m.grad_slots)
        CHECK(s.key.find("time_mlp.") == std::string::npos, "%s: %s entered dad_train_grad_info", a.name, s.key.c_str());

    const int Hr = traj_horizon(m);
    for (int B : {1, 5, 9, 250, 256, 512}) {
        ObjectiveLayout o;
        rc = objective_layout(m, B, o);
        CHECK(rc == DAD_OK, "%s B=%d: objective_layout: %s", a.name, B, g_err);
        // the existing parts: exactly what dad_train_workspace_bytes reports, rounded up to 256 bytes
        FwdPlan f;
        plan_forward(m, true, B, false, f);
        TrainScratch ts;
        train_scratch(m, B, ts);
        CHECK(o.saved_base >= f.bytes && o.saved_base < f.bytes + 256 && o.saved_base % 256 == 0, "%s B=%d: saved base %zu behind %zu", a.name, B,
              o.saved_base, f.bytes);
        const size_t old_scratch = (size_t)ts.total * sizeof(float);
        CHECK(o.scratch_base >= old_scratch && o.scratch_base < old_scratch + 256 && o.scratch_base % 256 == 0, "%s B=%d: scratch base %zu behind %zu",
              a.name, B, o.scratch_base, old_scratch);
        const long n = (long)B * Hr * c.transition_dim;
        // the reported sizes, derived here from the tensors' own shapes: the existing part rounded up to 256 bytes, then
        // every region rounded up to 64 floats (the last region's end is the end of the workspace)
        auto al64 = [](long v) { return (v + 63) / 64 * 64; };
        const long loss_blocks = std::max(1L, std::min(1024L, (n + 1023) / 1024));
        const long want_saved = 2 * al64(n) + 2 * al64(B) + al64(B * 4 * tdm) + 2 * al64(B * tdm) + al64((long)B * W) + al64(loss_blocks);
        CHECK(o.saved_bytes == (f.bytes + 255) / 256 * 256 + (size_t)want_saved * sizeof(float), "%s B=%d: saved %zu bytes", a.name, B, o.saved_bytes);
        CHECK(o.partial + al64(o.loss_blocks) == o.saved_floats, "%s B=%d: saved regions end at %ld of %ld", a.name, B, o.partial + al64(o.loss_blocks), o.saved_floats);
        CHECK(o.dh1 + al64(B * 4 * tdm) == o.scratch_floats, "%s B=%d: scratch regions end at %ld of %ld", a.name, B, o.dh1 + al64(B * 4 * tdm), o.scratch_floats);
        CHECK(o.loss_blocks >= 1 && o.loss_blocks <= kObjectiveMaxLossBlocks, "%s B=%d: %d loss blocks", a.name, B, o.loss_blocks);
        // K slices of d act
        CHECK(o.kslice > 0 && o.kslice % 128 == 0, "%s B=%d: K slice of %d columns", a.name, B, o.kslice);
        CHECK(o.kslices >= 1 && (long)(o.kslices - 1) * o.kslice < W && (long)o.kslices * o.kslice >= W, "%s B=%d: %d slices of %d over %d", a.name, B,
              o.kslices, o.kslice, W);
        std::vector<int> covered((size_t)W, 0);
        for (int z = 0; z < o.kslices; ++z) {
            const int kbeg = z * o.kslice, kend = std::min(W, kbeg + o.kslice);
            for (int k0 = kbeg; k0 < kend; k0 += 32) {              // a wave's chunk: one block's rows only
                int blk = 0;
                while (blk + 1 < (int)blocks.size() && blocks[blk + 1].off <= k0) ++blk;
                const int last = std::min(kend, k0 + 32) - 1;
                CHECK(k0 >= blocks[blk].off && last < blocks[blk].off + blocks[blk].cout, "%s B=%d: chunk [%d, %d] straddles block %d", a.name, B, k0,
                      last, blk);
                for (int k = k0; k <= last; ++k) ++covered[(size_t)k];
            }
        }
        for (int k = 0; k < W; ++k) CHECK(covered[(size_t)k] == 1, "%s B=%d: column %d in %d slices", a.name, B, k, covered[(size_t)k]);
        check_regions(a.name, B, "saved",
                      {{"xt", o.xt, n}, {"out", o.out, n}, {"t_rows", o.t_rows, B}, {"row_index", o.row_index, B},
                       {"h1", o.h1, B * 4 * tdm}, {"temb", o.temb, B * tdm}, {"act", o.act, B * tdm}, {"rows", o.rows, (long)B * W},
                       {"partial", o.partial, o.loss_blocks}},
                      o.saved_floats);
        const long want_scratch = al64(n) + al64((long)B * W) + al64((long)o.kslices * B * tdm) + al64(B * tdm) + al64(B * 4 * tdm);
        CHECK(o.scratch_bytes == (old_scratch + 255) / 256 * 256 + (size_t)want_scratch * sizeof(float), "%s B=%d: scratch %zu bytes", a.name, B, o.scratch_bytes);
        check_regions(a.name, B, "scratch",
                      {{"d_out", o.d_out, n}, {"d_rows", o.d_rows, (long)B * W}, {"dact_slab", o.dact_slab, (long)o.kslices * B * tdm},
                       {"dtemb", o.dtemb, B * tdm}, {"dh1", o.dh1, B * 4 * tdm}},
                      o.scratch_floats);
    }
    printf("  %-14s %2zu blocks, temb_width %5d, %zu time gradient tensors\n", a.name, blocks.size(), W, m.time_grad_slots.size());
}

int main() {
    const std::vector<Arch> archs = {
        {"tiny", 6, 32, 32, 32, {1, 2, 4}, {}, 0},
        {"tiny4", 8, 32, 32, 32, {1, 2, 2, 4}, {}, 0},
        {"tiny_td64", 6, 32, 64, 32, {1, 2, 4}, {}, 0},
        {"pointmaze", 6, 128, 128, 32, {1, 2, 4}, {}, 0},
        {"halfcheetah", 23, 256, 256, 32, {1, 4, 8}, {}, 0},
        {"d48_padded", 6, 64, 48, 32, {1, 2}, {48, 96}, 0},
        {"h24_padded", 6, 32, 32, 32, {1, 2, 4}, {}, 24},
    };
    for (const Arch& a : archs) check_arch(a);
    if (g_failures) { printf("%d failures\n", g_failures); return 1; }
    printf("objective host logic ok\n");
    return 0;
}
