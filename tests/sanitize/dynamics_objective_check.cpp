// dynamics_objective_check.cpp — the host planner of the dynamics-aware objective (csrc/host_plan.hpp
// dynamics_objective_plan; dad_train_dynamics_objective_forward / _backward), walked without HIP under
// -fsanitize=address,undefined against what the kernels of csrc/train_objective.hpp assume:
//   * its own regions of `saved` and `scratch` start behind the fused objective's, at multiples of 16 bytes, hold what
//     the kernels write into them, do not overlap, and end at the sizes dad_train_dynamics_objective_workspace_bytes reports;
//   * the fused objective's sizes are untouched;
//   * the form, the grids and the LDS sizes are plan_violation_grad's for x0_hat's shape, the launches come in launch
//     order, and the report encodes exactly them;
//   * the gather (dynamics_gather) and scatter (vg_dx_elem through dynamics_store_dout) index arithmetic, repeated here
//     for the first, an interior and the last trajectory: every read of x_t / out and every write of d_out stays inside
//     (B, H, td) — replayed into byte maps of exactly that size, which the sanitizer watches —; the entries of g a d_out
//     element consumes (a map of exactly D entries) are the ones the gather reads from that element, each consumed
//     once, the last state's two; and every element of r, the partial sums and g is written once by the grids planned.
// Built and run by tests/test_dynamics_objective_host.py (CPU suite).
#include <cstdio>
#include <vector>

#include "../../dynamics_aware_diffusion_amd/csrc/plan_report.hpp"

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

struct Region { const char* name; long at, floats; };

static void check_regions(const char* what, const std::vector<Region>& rs, long total) {
    std::vector<unsigned char> owner((size_t)total, 0);
    int id = 0;
    for (const Region& r : rs) {
        ++id;
        if (r.floats == 0) continue;
        CHECK(r.at >= 0 && r.at + r.floats <= total, "%s.%s: [%ld, %ld) of %ld", what, r.name, r.at, r.at + r.floats, total);
        CHECK((r.at * (long)sizeof(float)) % 16 == 0, "%s.%s: offset %ld floats is not 16-byte aligned", what, r.name, r.at);
        if (r.at < 0 || r.at + r.floats > total) continue;
        for (long i = r.at; i < r.at + r.floats; ++i) {
            CHECK(owner[(size_t)i] == 0, "%s.%s overlaps region %d at float %ld", what, r.name, (int)owner[(size_t)i], i);
            if (owner[(size_t)i] != 0) break;
            owner[(size_t)i] = (unsigned char)id;
        }
    }
}

// dynamics_gather's index of element d (0 .. D-1) of trajectory b into (B, H, td) (train_objective.hpp)
static long gather_index(int b, int d, int H, int n, int od, int m, int td) {
    const int nstate = (H + 1) * n;
    int ts, c;
    if (d < nstate) {
        ts = d / n;
        c = d - ts * n;
        if (ts >= H) ts = H - 1;
    } else {
        const int dd = d - nstate;
        ts = dd / m;
        c = od + (dd - ts * m);
    }
    return ((long)b * H + ts) * td + c;
}

static void check_case(const HostModel& m, const char* arch, int B, int n, int mm, int form) {
    const int od = n, td = m.cfg.transition_dim, H = traj_horizon(m);
    DynamicsObjectivePlan p;
    const int rc = dynamics_objective_plan(m, B, n, od, mm, form, true, p);
    CHECK(rc == DAD_OK, "%s B=%d n=%d m=%d form=%d: %s", arch, B, n, mm, form, g_err);
    if (rc != DAD_OK) return;
    const int D = (H + 1) * n + H * mm;
    CHECK(p.D == D && p.horizon == H, "%s: D %d (want %d), horizon %d (want %d)", arch, p.D, D, p.horizon, H);
    const ViolationGradPlan vg = plan_violation_grad(D, B, (long)H * td, form);
    CHECK(p.vg.form == vg.form && p.vg.refused == vg.refused && p.vg.col_blocks == vg.col_blocks, "%s B=%d: form %d, the violation pair plans %d", arch,
          B, p.vg.form, vg.form);
    const bool gemm = p.vg.form == DAD_VG_GEMM;
    // the fused objective's sizes, untouched, and this step's behind them
    ObjectiveLayout o;
    objective_layout(m, B, o);
    CHECK(p.saved_base >= o.saved_bytes && p.saved_base < o.saved_bytes + 256 && p.saved_base % 256 == 0, "%s B=%d: saved base %zu behind %zu", arch, B,
          p.saved_base, o.saved_bytes);
    CHECK(p.scratch_base >= o.scratch_bytes && p.scratch_base < o.scratch_bytes + 256 && p.scratch_base % 256 == 0, "%s B=%d: scratch base %zu behind %zu",
          arch, B, p.scratch_base, o.scratch_bytes);
    CHECK(p.obj.o.saved_bytes == o.saved_bytes && p.obj.o.scratch_bytes == o.scratch_bytes, "%s B=%d: the objective's own sizes moved", arch, B);
    CHECK(p.saved_bytes == p.saved_base + (size_t)p.saved_floats * 4 && p.scratch_bytes == p.scratch_base + (size_t)p.scratch_floats * 4, "%s B=%d: totals", arch, B);
    const long bd = (long)B * D;
    check_regions("saved", {{"r", p.r, bd}, {"part", p.part, gemm ? (long)B * p.vg.col_blocks : 0}, {"violation", p.violation, gemm ? 0 : B}}, p.saved_floats);
    check_regions("scratch", {{"g", p.g, gemm ? bd : 0}}, p.scratch_floats);
    // launches, in order, with the violation pair's grids
    const size_t want = gemm ? 4 : 3;
    CHECK(p.launches.size() == want && p.fwd_launches == 2, "%s B=%d: %zu launches", arch, B, p.launches.size());
    if (p.launches.size() != want) return;
    const DynLaunch &f = p.launches[0], &parts = p.launches[1], &b = p.launches[2];
    CHECK(f.kind == (gemm ? DAD_DO_K_FWD_GEMM : DAD_DO_K_FWD_ROW) && parts.kind == DAD_DO_K_FWD_PARTS && b.kind == (gemm ? DAD_DO_K_BWD_GEMM : DAD_DO_K_BWD_ROW),
          "%s B=%d: kinds %d %d %d", arch, B, f.kind, parts.kind, b.kind);
    CHECK(f.gx == vg.fwd.gx && f.gy == vg.fwd.gy && f.lds_bytes == vg.fwd.lds_bytes && b.gx == vg.bwd.gx && b.gy == vg.bwd.gy && b.lds_bytes == vg.bwd.lds_bytes,
          "%s B=%d: grids differ from the violation pair's", arch, B);
    CHECK(parts.gx == 1 && parts.gy == 1 && parts.threads == 256, "%s B=%d: the parts launch is one block of 256", arch, B);
    if (!p.vg.refused) CHECK(f.lds_bytes <= dad::kLdsBytes && b.lds_bytes <= dad::kLdsBytes, "%s B=%d: LDS %zu / %zu", arch, B, f.lds_bytes, b.lds_bytes);
    {
        std::vector<int32_t> rep;
        const int rrc = dynamics_objective_plan_report(m, B, n, od, mm, form, rep);
        CHECK(rrc == rc && rep.size() == (size_t)DAD_DO_HEADER + want * DAD_DO_REC_INTS && rep[DAD_DO_LAUNCHES] == (int32_t)want && rep[DAD_DO_FORM] == p.vg.form,
              "%s B=%d: report of %zu ints", arch, B, rep.size());
    }
    // which elements of r / part / g the planned grids write (the kernels' own guards: b < B, d < D), once each
    const int rpb = f.rows_per_block;
    std::vector<unsigned char> r_hit((size_t)bd, 0);
    if (gemm) {
        std::vector<unsigned char> part_hit((size_t)B * p.vg.col_blocks, 0), g_hit((size_t)bd, 0);
        for (unsigned bx = 0; bx < f.gx; ++bx)
            for (unsigned by = 0; by < f.gy; ++by)
                for (int r = 0; r < 32; ++r) {
                    const int bb = (int)bx * 32 + r;
                    if (bb >= B) continue;
                    ++part_hit.at((size_t)bb * p.vg.col_blocks + by);
                    for (int c = 0; c < 32; ++c) {
                        const int d = (int)by * 32 + c;
                        if (d < D) { ++r_hit.at((size_t)bb * D + d); ++g_hit.at((size_t)bb * D + d); }
                    }
                }
        for (unsigned char c : part_hit) CHECK(c == 1, "%s B=%d: a partial sum written %d times", arch, B, c);
        for (unsigned char c : g_hit) CHECK(c == 1, "%s B=%d: an element of g written %d times", arch, B, c);
        const DynLaunch& s = p.launches[3];
        const long n_out = (long)B * H * td;
        CHECK(s.kind == DAD_DO_K_BWD_SCATTER && (long)s.gx * s.threads >= n_out && (long)(s.gx - 1) * s.threads < n_out, "%s B=%d: scatter grid %u", arch, B, s.gx);
    } else {
        CHECK(rpb == 1 || rpb == 4, "%s B=%d: %d trajectories per block", arch, B, rpb);
        CHECK((long)f.gx * rpb >= B && (long)(f.gx - 1) * rpb < B && b.gx == (unsigned)B, "%s B=%d: row grids %u / %u", arch, B, f.gx, b.gx);
        for (unsigned bx = 0; bx < f.gx; ++bx)
            for (int r = 0; r < rpb; ++r) {
                const int bb = (int)bx * rpb + r;
                if (bb >= B) continue;
                for (int d = 0; d < D; ++d) ++r_hit.at((size_t)bb * D + d);
            }
    }
    for (unsigned char c : r_hit) CHECK(c == 1, "%s B=%d: an element of r written %d times", arch, B, c);
    // gather / scatter index arithmetic for the first, an interior and the last trajectory
    const long n_out = (long)B * H * td;
    std::vector<unsigned char> read((size_t)n_out, 0), written((size_t)n_out, 0);
    const int picks[3] = {0, B / 2, B - 1};
    for (int k = 0; k < 3; ++k) {
        const int bb = picks[k];
        if (k > 0 && bb == picks[k - 1]) continue;
        for (int d = 0; d < D; ++d) {
            const long i = gather_index(bb, d, H, n, od, mm, td);
            CHECK(i >= (long)bb * H * td && i < (long)(bb + 1) * H * td, "%s B=%d: element %d of trajectory %d gathers from %ld", arch, B, d, bb, i);
            ++read.at((size_t)i);
        }
        // the scatter is the transpose of the gather: the entries of g that element e = ts * td + c of d_out consumes
        // (vg_dx_elem: g[ts n + c], and g[H n + c] too at the last step; none for an observation channel past the
        // state; g[(H + 1) n + ts m + k] for action k), marked in a map of exactly D entries, are the d the gather
        // reads from that very element; every entry of g is consumed once
        std::vector<unsigned char> g_used((size_t)D, 0);
        for (int e = 0; e < H * td; ++e) {
            const int ts = e / td, c = e - ts * td;
            int gi[2], ng = 0;
            if (c < n) {
                gi[ng++] = ts * n + c;
                if (ts == H - 1) gi[ng++] = H * n + c;
            } else if (c >= od) {
                gi[ng++] = (H + 1) * n + ts * mm + (c - od);
            }
            for (int k = 0; k < ng; ++k) {
                ++g_used.at((size_t)gi[k]);
                CHECK(gather_index(bb, gi[k], H, n, od, mm, td) == (long)bb * H * td + e, "%s B=%d: d_out element %d of trajectory %d consumes g[%d], which "
                      "the gather reads from element %ld", arch, B, e, bb, gi[k], gather_index(bb, gi[k], H, n, od, mm, td) - (long)bb * H * td);
            }
            CHECK(ng == (c < n ? (ts == H - 1 ? 2 : 1) : c < od ? 0 : 1), "%s B=%d: d_out element %d consumes %d entries of g", arch, B, e, ng);
            ++written.at((size_t)((long)bb * H * td + e));        // (dynamics_store_dout's index: b * row_elems + e)
        }
        for (int d = 0; d < D; ++d) CHECK(g_used[(size_t)d] == 1, "%s B=%d: g[%d] of trajectory %d consumed %d times", arch, B, d, bb, g_used[(size_t)d]);
        for (int e = 0; e < H * td; ++e) {
            const size_t i = (size_t)((long)bb * H * td + e);
            const int c = e % td;
            CHECK(written[i] == 1, "%s B=%d: d_out element %d of trajectory %d written %d times", arch, B, e, bb, written[i]);
            // every state / action channel is gathered (the last state twice), observation channels past the state never
            const int ts = e / td;
            const int want_reads = c < n ? (ts == H - 1 ? 2 : 1) : c < od ? 0 : 1;
            CHECK(read[i] == want_reads, "%s B=%d: x0_hat element %d of trajectory %d gathered %d times", arch, B, e, bb, read[i]);
        }
    }
}

struct Arch { const char* name; int n, m, dim, horizon, hreal; std::vector<int> mults; };

int main() {
    const std::vector<Arch> archs = {
        {"n4m2_H32", 4, 2, 32, 32, 0, {1, 2, 4}},
        {"n4m2_H8", 4, 2, 32, 8, 0, {1, 2}},
        {"n4m2_H24", 4, 2, 32, 32, 24, {1, 2, 4}},        // zero-padded horizon: the trajectories have 24 steps
        {"n17m6_H32", 17, 6, 32, 32, 0, {1, 2, 4}},
        {"n17m6_H8", 17, 6, 32, 8, 0, {1, 2}},
        {"n39m28_H32", 39, 28, 32, 32, 0, {1, 2, 4}},     // D = 2183: the planner takes the GEMM form from batch 32
        {"n39m28_H24", 39, 28, 32, 32, 24, {1, 2, 4}},
    };
    for (const Arch& a : archs) {
        HostModel m;
        dad_cfg& c = m.cfg;
        c.transition_dim = a.n + a.m; c.dim = a.dim; c.time_dim = a.dim;
        c.n_levels = (int)a.mults.size();
        for (size_t i = 0; i < a.mults.size(); ++i) c.channels[i] = a.dim * a.mults[i];
        c.kernel_size = 5; c.horizon = a.horizon; c.n_timesteps = 20;
        c.predict_epsilon = c.clip_denoised = 1;
        int rc = check_cfg(&c);
        CHECK(rc == DAD_OK, "%s: check_cfg: %s", a.name, g_err);
        if (rc != DAD_OK) continue;
        m.real_horizon = a.hreal;
        m.training = true;
        rc = build_plan(&m);
        CHECK(rc == DAD_OK, "%s: build_plan: %s", a.name, g_err);
        if (rc != DAD_OK) continue;
        int cases = 0;
        for (int B : {1, 3, 32, 33, 256})
            for (int form : {-1, 0, 1}) { check_case(m, a.name, B, a.n, a.m, form); ++cases; }
        // refusals of the shape come back with a message and plan nothing
        DynamicsObjectivePlan p;
        CHECK(dynamics_objective_plan(m, 0, a.n, a.n, a.m, -1, true, p) == DAD_E_INVALID && p.launches.empty(), "%s: batch 0", a.name);
        CHECK(dynamics_objective_plan(m, 4, a.n, a.n, a.m, 2, true, p) == DAD_E_INVALID && p.launches.empty(), "%s: form 2", a.name);
        CHECK(dynamics_objective_plan(m, 4, a.n, a.n, a.m + 1, -1, true, p) == DAD_E_INVALID && p.launches.empty(), "%s: widths", a.name);
        CHECK(dynamics_objective_plan(m, 4, a.n + 1, a.n, a.m, -1, true, p) == DAD_E_INVALID && p.launches.empty(), "%s: state_dim", a.name);
        printf("  %-12s D = %4d, %d cases\n", a.name, (traj_horizon(m) + 1) * a.n + traj_horizon(m) * a.m, cases);
    }
    if (g_failures) { printf("%d failures\n", g_failures); return 1; }
    printf("dynamics objective host logic ok\n");
    return 0;
}
