// objective_check.cpp — the workspace layout of the fused training objective (csrc/host_plan.hpp objective_layout;
// dad_train_objective_forward / dad_train_objective_backward), walked on the host without HIP under
// -fsanitize=address,undefined against what the kernels of csrc/train_objective.hpp assume:
//   * the new regions of `saved` and `scratch` start behind the existing parts, at multiples of 16 bytes, hold what
//     the kernels write into them, do not overlap, and end at the sizes dad_train_objective_workspace_bytes reports;
//   * the existing sizes (dad_train_workspace_bytes) are untouched;
//   * the K slices of d act = d rows . W cover temb_width exactly once in whole 128-column steps (32 per wave), and a
//     32-column chunk never straddles two ResidualTemporalBlocks;
//   * the time gradient list names every time-MLP tensor once, at aligned offsets, with the element counts of the
//     expected shapes;
//   * the nine launches of the time chain (ObjectivePlan::time, what the two entry points replay) come in launch order,
//     their grids cover their outputs in 32 x 32 tiles, and every launch writes exactly the region of the layout (or
//     the gradient slots) it is given: each store of time_gemm_kernel / time_dtemb_kernel is replayed into a byte map
//     of that region the sanitizer watches.
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

// Every element a launch stores, as the kernels index them (train_objective.hpp: out[i * N + j] for i < M, j < N of
// the tiles of the grid; TG_BWD_DACT: slab blockIdx.z; weight gradients of the blocks: rows relative to the block's
// first; bias gradients: one per row), replayed into maps of exactly the destination's size.
static void check_time_launches(const Arch& a, const HostModel& m, int B, const ObjectivePlan& p) {
    const ObjectiveLayout& o = p.o;
    const long tdm = m.cfg.time_dim;
    const int W = m.tplan.temb_width;
    const std::vector<TimeBlockRef> blocks = time_block_list(m);
    static const int order[kObjectiveTimeLaunches] = {DAD_OP_TG_FWD_H1, DAD_OP_TG_FWD_TEMB, DAD_OP_TG_FWD_ROWS, DAD_OP_TG_BWD_DWK, DAD_OP_TG_BWD_DACT,
                                                      DAD_OP_TG_DTEMB, DAD_OP_TG_BWD_DW3, DAD_OP_TG_BWD_DH1, DAD_OP_TG_BWD_DW1};
    CHECK(p.time.size() == (size_t)kObjectiveTimeLaunches, "%s B=%d: %zu time launches", a.name, B, p.time.size());
    if (p.time.size() != (size_t)kObjectiveTimeLaunches) return;
    auto slot = [&](size_t i) { return (long)m.time_grad_slots[i].numel; };
    // the float count of a saved / scratch region: up to the next region's start
    const long saved_regions[] = {o.xt, o.out, o.t_rows, o.row_index, o.h1, o.temb, o.act, o.rows, o.partial, o.saved_floats};
    const long scratch_regions[] = {o.d_out, o.d_rows, o.dact_slab, o.dtemb, o.dh1, o.scratch_floats};
    auto room = [&](const long* rs, size_t n, long at) {
        for (size_t i = 0; i + 1 < n; ++i) if (rs[i] == at) return rs[i + 1] - at;
        return -1L;
    };
    for (int li = 0; li < kObjectiveTimeLaunches; ++li) {
        const TimeLaunch& l = p.time[(size_t)li];
        CHECK(l.mode == order[li], "%s B=%d: launch %d is mode %d", a.name, B, li, l.mode);
        CHECK(l.M > 0 && l.N > 0 && l.K > 0 && l.kslice > 0 && l.kslices > 0, "%s B=%d launch %d: %d x %d x %d, %d x %d", a.name, B, li, l.M, l.N, l.K,
              l.kslices, l.kslice);
        if (l.M <= 0 || l.N <= 0 || l.K <= 0 || l.kslice <= 0 || l.kslices <= 0) continue;
        if (l.mode == DAD_OP_TG_DTEMB) {
            const long n = (long)l.M * l.N;
            CHECK(n == B * tdm && l.K == o.kslices && (long)l.gx() * 256 >= n && (long)(l.gx() - 1) * 256 < n && l.gy() == 1 && l.gz() == 1,
                  "%s B=%d: slab sum over %ld elements, %d slabs, grid %u", a.name, B, n, l.K, l.gx());
            CHECK((long)l.K * n <= room(scratch_regions, 6, o.dact_slab) && n <= room(scratch_regions, 6, o.dtemb) && n <= room(saved_regions, 10, o.temb),
                  "%s B=%d: slab sum reads %d x %ld floats", a.name, B, l.K, n);
            continue;
        }
        // the K slices cover K once, in whole chunks per wave except in the last slice
        CHECK((long)(l.kslices - 1) * l.kslice < l.K && (long)l.kslices * l.kslice >= l.K && (l.kslices == 1 || l.kslice % 32 == 0),
              "%s B=%d launch %d: %d slices of %d over K = %d", a.name, B, li, l.kslices, l.kslice, l.K);
        CHECK(l.gx() == (unsigned)((l.M + 31) / 32) && l.gy() == (unsigned)((l.N + 31) / 32) && l.gz() == (unsigned)l.kslices, "%s B=%d launch %d: grid", a.name,
              B, li);
        // destination(s): {name, floats the destination holds, writes}
        long want = 0, want2 = -1, have = -1;
        switch (l.mode) {
            case DAD_OP_TG_FWD_H1: want = B * 4 * tdm; have = room(saved_regions, 10, o.h1); CHECK(l.K == m.cfg.dim, "%s: K of h1", a.name); break;
            case DAD_OP_TG_FWD_TEMB:
                want = B * tdm; have = std::min(room(saved_regions, 10, o.temb), room(saved_regions, 10, o.act));
                CHECK(l.K == 4 * tdm, "%s: K of temb", a.name);
                break;
            case DAD_OP_TG_FWD_ROWS: want = (long)B * W; have = room(saved_regions, 10, o.rows); CHECK(l.K == tdm, "%s: K of rows", a.name); break;
            case DAD_OP_TG_BWD_DACT:
                want = (long)o.kslices * B * tdm; have = room(scratch_regions, 6, o.dact_slab);
                CHECK(l.K == W && l.kslice == o.kslice && l.kslices == o.kslices, "%s B=%d: d act slices %d x %d, layout %d x %d", a.name, B, l.kslices, l.kslice,
                      o.kslices, o.kslice);
                break;
            case DAD_OP_TG_BWD_DH1: want = B * 4 * tdm; have = room(scratch_regions, 6, o.dh1); CHECK(l.K == tdm, "%s: K of d h1", a.name); break;
            case DAD_OP_TG_BWD_DW3: want = have = slot(2); want2 = slot(3); CHECK(l.K == B, "%s: K of d W3", a.name); break;
            case DAD_OP_TG_BWD_DW1: want = have = slot(0); want2 = slot(1); CHECK(l.K == B, "%s: K of d W1", a.name); break;
            default: break;
        }
        if (l.mode == DAD_OP_TG_BWD_DWK) {
            // per block: rows [off, off + cout) of the M = temb_width rows go to the block's own weight / bias gradient
            CHECK(l.M == W && l.N == tdm && l.K == B, "%s B=%d: d Wk is %d x %d over %d", a.name, B, l.M, l.N, l.K);
            std::vector<std::vector<unsigned char>> dw(blocks.size()), db(blocks.size());
            for (size_t k = 0; k < blocks.size(); ++k) { dw[k].assign((size_t)slot(4 + 2 * k), 0); db[k].assign((size_t)slot(5 + 2 * k), 0); }
            for (unsigned bx = 0; bx < l.gx(); ++bx) {
                int blk = 0;
                while (blk + 1 < (int)blocks.size() && blocks[(size_t)blk + 1].off <= (int)bx * 32) ++blk;
                for (int i = (int)bx * 32; i < std::min(l.M, (int)bx * 32 + 32); ++i) {
                    const long row = i - blocks[(size_t)blk].off;
                    CHECK(row >= 0 && row < blocks[(size_t)blk].cout, "%s B=%d: row %d of d Wk leaves block %d", a.name, B, i, blk);
                    if (row < 0 || row >= blocks[(size_t)blk].cout) continue;
                    for (int j = 0; j < l.N; ++j) ++dw[(size_t)blk].at((size_t)(row * l.N + j));
                    ++db[(size_t)blk].at((size_t)row);
                }
            }
            for (size_t k = 0; k < blocks.size(); ++k) {
                for (unsigned char c : dw[k]) CHECK(c == 1, "%s B=%d: an element of %s.time_mlp.1.weight.grad written %d times", a.name, B, blocks[k].base.c_str(), c);
                for (unsigned char c : db[k]) CHECK(c == 1, "%s B=%d: an element of %s.time_mlp.1.bias.grad written %d times", a.name, B, blocks[k].base.c_str(), c);
            }
            continue;
        }
        CHECK(have >= 0 && want <= have, "%s B=%d launch %d (mode %d): writes %ld floats into %ld", a.name, B, li, l.mode, want, have);
        if (have < 0 || want > have) continue;
        std::vector<unsigned char> hit((size_t)want, 0);
        for (unsigned z = 0; z < l.gz(); ++z)
            for (unsigned bx = 0; bx < l.gx(); ++bx)
                for (unsigned by = 0; by < l.gy(); ++by)
                    for (int i = (int)bx * 32; i < std::min(l.M, (int)bx * 32 + 32); ++i)
                        for (int j = (int)by * 32; j < std::min(l.N, (int)by * 32 + 32); ++j)
                            ++hit.at((size_t)((l.mode == DAD_OP_TG_BWD_DACT ? (long)z * l.M + i : (long)i) * l.N + j));
        for (unsigned char c : hit) CHECK(c == 1, "%s B=%d launch %d (mode %d): an output element written %d times", a.name, B, li, l.mode, c);
        if (want2 >= 0) CHECK(want2 == l.M, "%s B=%d launch %d: %d bias gradients into %ld", a.name, B, li, l.M, want2);
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
        ObjectivePlan op;
        rc = objective_plan(m, B, true, op);
        const ObjectiveLayout& o = op.o;
        CHECK(rc == DAD_OK, "%s B=%d: objective_plan: %s", a.name, B, g_err);
        check_time_launches(a, m, B, op);
        {
            std::vector<int32_t> rep;
            CHECK(objective_plan_report(m, B, rep) == rc && rep.size() == (size_t)(DAD_OP_HEADER + kObjectiveTimeLaunches * DAD_OP_REC_INTS),
                  "%s B=%d: report of %zu ints", a.name, B, rep.size());
        }
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
        {"tiny_td20", 6, 32, 20, 32, {1, 2, 4}, {}, 0},       // time_dim no multiple of the 32-wide tile
        {"tiny_td72", 6, 32, 72, 32, {1, 2, 4}, {}, 0},
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
