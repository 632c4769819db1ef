// seam_check.cpp — the host side of csrc/conv_seam.hpp (the posterior update of step t and the first conv of step
// t - 1 as one launch), checked without HIP under -fsanitize=address,undefined:
//   * plan_seam's rule over a sweep of (transition_dim 1..20, dim, horizon, batch, options) against a restatement of
//     it, every refusal with a reason of its own, and the buffer condition on hand-made plans;
//   * the kernel's LDS regions (conv_shapes.hpp seam_lds_floats) are disjoint, 16-byte aligned and inside the
//     allocation; every address the kernel forms stays inside its region;
//   * a simulated X stage (zero fill, then the posterior's stores, tagged) returns to every fragment read exactly the
//     (sample, position + tap - 2, channel) element of the conv, or a zero: halo rows, channels >= transition_dim,
//     samples beyond the batch; with slot shifts every ds_read_b128 group of 16 lanes hits 16 distinct slots;
//   * the unit left out when transition_dim <= 8 reads zeros only;
//   * the two float4 of every thread lie in one (sample, group) pair, the threads cover the tile exactly once, and
//     the leaves of a pair are the leaves of conv_gemm_f32's reduction for the tile the launch stands in for.
// The kernel's address arithmetic is repeated here from its source.  Built and run by tests/test_hip_seam.py.
#include <cstdio>
#include <set>
#include <vector>

#include "../../dynamics_aware_diffusion_amd/csrc/host_plan.hpp"

using namespace dadhost;

static int g_failures = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            if (++g_failures <= 40) {                                                     \
                fprintf(stderr, "CHECK failed %s:%d: %s — ", __FILE__, __LINE__, #cond);  \
                fprintf(stderr, __VA_ARGS__);                                             \
                fprintf(stderr, "\n");                                                    \
            }                                                                             \
        }                                                                                 \
    } while (0)

static long g_reads = 0;

static bool build(HostModel& m, int td, int dim, std::vector<int> mults, int horizon, int ksize = 5) {
    dad_cfg& c = m.cfg;
    c.transition_dim = td; c.dim = dim; c.time_dim = dim;
    c.n_levels = (int)mults.size();
    for (size_t i = 0; i < mults.size(); ++i) c.channels[i] = dim * mults[i];
    c.kernel_size = ksize; c.horizon = horizon; c.n_timesteps = 20;
    c.predict_epsilon = c.clip_denoised = 1;
    if (check_cfg(&c) != DAD_OK) return false;
    return build_plan(&m) == DAD_OK;
}

// ---- the kernel's LDS arithmetic for one (dim, horizon, transition_dim, tile, batch tail) -------------------------
static void check_kernel(const HostModel& probe, int DIM, int H, int td, bool T0, int nvalid_last, bool shifts) {
    constexpr int KP = dad::SEAM_KP, PAD = 2, TAPS = 5;
    const int NT = dad::seam_threads(DIM), TMW = DIM / 32, ES = DIM + 4, JG = NT / 32, JB = 16 / JG, DQ = DIM / 4;
    const int hsh = ilog2(H), SPT = 32 >> hsh, SEG = H + 2 * PAD, XF = dad::seam_xf(H);
    const int units = td > 8 ? 2 : 1;
    const uint64_t xswz = shifts ? find_xswz(probe, H, 1, PAD, KP / 4, 32) : 0;
    if (shifts && H < 32) CHECK(xswz != 0, "no slot shifts for H = %d, KP = %d", H, KP);
    auto shift = [&](int s) { return (int)((xswz >> (4 * s)) & 15) * 4; };
    // regions
    const long total = (long)dad::seam_lds_floats(td, DIM, H);
    const long o_tile = 0, o_wl = o_tile + 32 * ES, o_bl = o_wl + (long)td * DIM, o_xs = o_bl + ((td + 3) & ~3), o_er = o_xs + XF;
    CHECK(o_er + 32 * ES == total, "dim %d H %d td %d: the regions end at %ld of %ld floats", DIM, H, td, o_er + 32 * ES, total);
    for (long o : {o_wl, o_bl, o_xs, o_er}) CHECK(o % 4 == 0, "region offset %ld is not 16-byte aligned", o);
    CHECK((size_t)total * sizeof(float) <= dad::kLdsBytes, "dim %d: %ld floats of LDS", DIM, total);
    CHECK(NT <= 1024 && NT % 64 == 0 && NT / 64 == 2 * TMW && JB * JG == 16, "dim %d: %d threads", DIM, NT);
    CHECK(2 * NT * 4 == 32 * DIM && td * DQ <= NT && td <= NT, "dim %d: staging items per thread", DIM);
    for (int s = 0; s + 1 < SPT; ++s)
        CHECK(shift(s) / 4 - shift(s + 1) / 4 <= PAD * (KP / 4), "H %d: shift pushes sample %d onto its neighbour", H, s);
    // the X stage as the kernel fills it: -1 zero, else tag (row, channel)
    std::vector<int> xs((size_t)XF, -2);
    for (int i = 0; i < (XF >> 2); ++i) for (int e = 0; e < 4; ++e) xs[(size_t)i * 4 + e] = -1;
    for (int v : xs) CHECK(v == -1, "the zero fill leaves a word of the stage unwritten");
    std::vector<int> xcount((size_t)32 * 16, 0);
    for (int tid = 0; tid < NT; ++tid) {
        const int col = tid & 31, jg = tid >> 5;
        const int s = col >> hsh, l = col & (H - 1);
        if (s >= nvalid_last) continue;                     // n >= N: rows of samples beyond the batch
        for (int k = 0; k < JB; ++k) {
            const int j = jg + k * JG;
            if (j >= td) continue;
            const int at = (s * SEG + PAD + l) * KP + shift(s) + j;
            CHECK(at >= 0 && at < XF, "posterior store at %d outside the X stage", at);
            if (at < 0 || at >= XF) continue;
            CHECK(xs[(size_t)at] == -1, "posterior store of (%d, %d, %d) lands on another element", s, l, j);
            xs[(size_t)at] = (s * H + l) * 16 + j;
            xcount[(size_t)col * 16 + j]++;
        }
    }
    for (int col = 0; col < 32; ++col)
        for (int j = 0; j < 16; ++j)
            CHECK(xcount[(size_t)col * 16 + j] == ((col >> hsh) < nvalid_last && j < td ? 1 : 0), "x element (%d, %d) written %d times", col, j,
                  xcount[(size_t)col * 16 + j]);
    // every fragment read of the conv waves (the ride reads tap PAD)
    for (int tap = 0; tap < TAPS; ++tap)
        for (int g = 0; g < 2; ++g) {
            int addr[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int l32 = lane & 31, h = lane >> 5;
                const int s = l32 >> hsh, l = l32 & (H - 1);
                const int arow4 = (((s * SEG + l) * KP + 4 * h) >> 2) + shift(s) / 4;
                const int a4 = arow4 + tap * (KP / 4) + g * 2;
                addr[lane] = a4 * 4;
                CHECK(a4 >= 0 && a4 * 4 + 4 <= XF, "fragment read at %d outside the X stage", a4 * 4);
                if (a4 < 0 || a4 * 4 + 4 > XF) continue;
                const int lsrc = l + tap - PAD;
                for (int e = 0; e < 4; ++e) {
                    const int ch = g * 8 + 4 * h + e;       // channel of chain e, k index h
                    const bool real = lsrc >= 0 && lsrc < H && ch < td && s < nvalid_last;
                    const int want = real ? (s * H + lsrc) * 16 + ch : -1;
                    CHECK(xs[(size_t)a4 * 4 + e] == want, "dim %d H %d td %d tap %d unit %d lane %d: stage holds %d, the conv reads %d", DIM, H, td,
                          tap, g, lane, xs[(size_t)a4 * 4 + e], want);
                    if (g >= units) CHECK(xs[(size_t)a4 * 4 + e] == -1, "the unit left out holds a real channel");
                }
                ++g_reads;
            }
            if (shifts)                                     // ds_read_b128: groups of 16 lanes, 16 slots of 16 bytes
                for (const auto& grp : {std::vector<int>{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                        std::vector<int>{4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}})
                    for (int h = 0; h < 2; ++h) {
                        std::set<int> slots;
                        for (int l32 : grp) slots.insert((addr[h * 32 + l32] >> 2) & 15);
                        CHECK(slots.size() == 16, "H %d tap %d unit %d: a fragment read hits %zu slots", H, tap, g, slots.size());
                    }
        }
    // weight fragments: lane (channel, k half) of unit g reads 16 bytes inside granule 0 of its tap slot
    for (int wave = 0; wave < 2 * TMW; ++wave)
        for (int lane = 0; lane < 64; ++lane)
            for (int slot = 0; slot <= TAPS; ++slot)
                for (int g = 0; g < 2; ++g) {
                    const int tm = wave >= TMW ? wave - TMW : wave;
                    const long at = (long)(tm * 32 + (lane & 31)) * 16 + 4 * (lane >> 5) + (long)slot * DIM * 16 + g * 8;
                    CHECK(at >= 0 && at + 4 <= (long)(TAPS + 1) * DIM * 16, "weight fragment at %ld outside granule 0", at);
                    CHECK(at % 16 / 4 == 2 * g + (lane >> 5), "weight fragment channels");
                }
    // exchange tile: accumulator register r of lane (l32, h) -> row, column
    std::vector<int> ehit((size_t)32 * DIM, 0);
    for (int tm = 0; tm < TMW; ++tm)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 16; ++r) {
                const int at = ((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * ES + tm * 32 + (lane & 31);
                CHECK(at >= 0 && at < 32 * ES, "exchange store at %d", at);
                if (at >= 0 && at < 32 * ES) ehit[(size_t)(at / ES) * DIM + at % ES]++;
            }
    for (int v : ehit) CHECK(v == 1, "exchange tile element written %d times", v);
    // epilogue ownership
    const int CPG = DIM / 8, CQ = CPG / 4, cq_sh = ilog2(CQ), cnt4 = H * CQ, lpp = T0 ? cnt4 : cnt4 >> 1, lpp_sh = ilog2(lpp);
    CHECK(lpp >= 2 && is_pow2(lpp), "lanes per pair %d", lpp);
    std::vector<int> own((size_t)32 * DQ, 0);
    // conv_gemm_f32's ownership for the tile: thread vt, float4 k -> (row, column) of a pair-local tile of SPT samples
    const int F4PL = T0 ? 1 : 2;
    for (int tid = 0; tid < NT; ++tid) {
        int pair[2];
        for (int k = 0; k < 2; ++k) {
            const int vt = T0 ? 2 * tid + k : tid;
            const int pr = vt >> lpp_sh, lp = vt & (lpp - 1), ps = pr >> 3, pg = pr & 7;
            const int j = T0 ? lp : lp + k * lpp;
            const int erow = ps * H + (j >> cq_sh), ecol = pg * CPG + (j & (CQ - 1)) * 4;
            CHECK(erow >= 0 && erow < 32 && ecol >= 0 && ecol + 4 <= DIM, "thread %d owns (%d, %d)", tid, erow, ecol);
            if (erow < 0 || erow >= 32 || ecol < 0 || ecol + 4 > DIM) continue;
            own[(size_t)erow * DQ + ecol / 4]++;
            pair[k] = (erow >> hsh) * 8 + ecol / CPG;
            CHECK(pair[k] == pr, "thread %d float4 %d lies in pair %d, its lanes reduce pair %d", tid, k, pair[k], pr);
            // the same element in that kernel: its thread's k-th float4 (k of F4PL) is j = lp + k * lpp of the pair
            const int kk = T0 ? 0 : k;
            CHECK(kk < F4PL && j == lp + kk * lpp && j < cnt4, "leaf order");
        }
        CHECK(pair[0] == pair[1], "thread %d spans two pairs", tid);
        // lanes of a pair are contiguous and aligned: the butterfly never leaves the pair
        const int phys = T0 ? lpp >> 1 : lpp;
        CHECK(phys <= 64 && (tid / phys) == (T0 ? (2 * tid) >> lpp_sh : tid >> lpp_sh), "pair lanes");
    }
    for (int v : own) CHECK(v == 1, "tile float4 owned %d times", v);
}

// ---- the rule, restated -------------------------------------------------------------------------------------------
struct Opt { bool seam = true, cc = false, fuse = true, proj = false, split = true; int force = -1, prec = DAD_PREC_FP32, real_h = 0; };

static int expect_why(const HostModel& m, const FwdPlan& f, const Opt& o, int td, int dim, int H, int mult0, int ksize) {
    if (!o.seam) return SEAM_OPTION;
    if (f.cc.ok) return SEAM_SMALL_BATCH;
    if (o.prec != DAD_PREC_FP32) return SEAM_PRECISION;
    if (o.force >= 0 || !o.split) return SEAM_FORCED_TILE;
    if (o.proj) return SEAM_PROJECTION;
    if (o.real_h > 0 && o.real_h != H) return SEAM_PADDED;
    if (H != 8 && H != 16 && H != 32) return SEAM_HORIZON;
    if (td > 16) return SEAM_TRANSITION_DIM;
    if (dim != 32 && dim != 64 && dim != 128) return SEAM_DIM;
    if (mult0 != 1 || ksize != 5) return SEAM_FIRST_CONV;
    if (!o.fuse) return SEAM_NO_RIDE;
    const int cfg = f.launches[0].g.cfg;
    if (cfg != 0 && cfg != 1) return SEAM_TILE;
    return SEAM_TAKEN;      // (LDS always fits at these sizes; the buffer condition is checked on hand-made plans)
}

static void check_rule() {
    int taken = 0, seen[SEAM_WHYS] = {0};
    for (int dim : {32, 64, 128, 256})
        for (int H : {8, 16, 32, 64})
            for (int td = 1; td <= 20; ++td) {
                if (td == dim) continue;                     // (an identity residual: no ride, covered by "no ride" below)
                for (int variant = 0; variant < 3; ++variant) {
                    const int mult0 = variant == 1 ? 2 : 1, ksize = variant == 2 ? 3 : 5;
                    if (variant && (td % 5 || H == 64)) continue;
                    HostModel m;
                    if (!build(m, td, dim, mult0 == 1 ? std::vector<int>{1, 2} : std::vector<int>{2, 2}, H, ksize)) continue;
                    for (int B : {1, 3, 5, 64, 256, 1500}) {
                        std::vector<Opt> opts(10);
                        opts[1].seam = false; opts[2].cc = true; opts[3].fuse = false; opts[4].proj = true; opts[5].force = 0;
                        opts[6].split = false; opts[7].prec = DAD_PREC_F16X3; opts[8].force = 4; opts[9].real_h = H - 2;
                        for (const Opt& o : opts) {
                            if (o.real_h || o.prec != DAD_PREC_FP32) if (B != 5 || td % 4) continue;   // (these rebuild the plan)
                            HostModel n;
                            HostModel& q = (o.real_h || o.prec != DAD_PREC_FP32) ? n : m;
                            if (&q == &n) {
                                n.real_horizon = o.real_h; n.precision = o.prec;
                                if (!build(n, td, dim, {1, 2}, H, ksize)) continue;
                                if (o.prec != DAD_PREC_FP32) decide_kernel_families(&n);
                            }
                            q.step_seam = o.seam; q.cc_enabled = o.cc; q.fuse_residual = o.fuse; q.force_tile = o.force; q.split_enabled = o.split;
                            FwdPlan f;
                            if (plan_forward(q, false, B, true, f) != DAD_OK) continue;
                            const SeamPlan s = plan_seam(q, f, o.proj);
                            const int want = expect_why(q, f, o, td, dim, H, mult0, ksize);
                            CHECK(s.why == want, "td %d dim %d H %d B %d opt %d variant %d: plan_seam says '%s', the rule '%s'", td, dim, H, B,
                                  (int)(&o - &opts[0]), variant, seam_reason(s.why), seam_reason(want));
                            seen[s.why]++;
                            if (!s.taken()) continue;
                            ++taken;
                            const LaunchGeom& g = f.launches[0].g;
                            CHECK(s.tile0 == (g.cfg == 0) && s.units == (td > 8 ? 2 : 1), "tile / units");
                            // the instantiation launch_seam looks up, by the key of its family
                            CHECK(seam_kernel_exists(q.cfg.dim, s.tile0) && family_kernel_exists(FAM_SEAM, {q.cfg.dim, s.tile0}),
                                  "td %d dim %d H %d B %d: conv_seam_f32<%d, tile0 %d> does not exist", td, dim, H, B, q.cfg.dim, (int)s.tile0);
                            CHECK(s.grid == (unsigned)(((long)B * H + 31) / 32) && s.threads == dad::seam_threads(dim), "grid %u, %d threads", s.grid, s.threads);
                            CHECK(s.lds_bytes == dad::seam_lds_floats(td, dim, H) * sizeof(float) && s.lds_bytes <= dad::kLdsBytes, "LDS %zu", s.lds_bytes);
                            CHECK(s.xswz == find_xswz(q, H, 1, 2, dad::SEAM_KP / 4, 32), "slot shifts");
                            // what the report adds, against the description it was read from
                            CHECK(s.dim == q.cfg.dim && s.spt * H == 32, "instantiation dim %d, %d samples per tile at H %d", s.dim, s.spt, H);
                            CHECK(s.last >= 1 && s.last <= s.spt && ((long)s.grid - 1) * s.spt + s.last == B, "B %d: %u tiles of %d, last %d", B,
                                  s.grid, s.spt, s.last);
                            {
                                const ConvOp& fop = q.plan.convs[f.launches[0].conv];
                                const int fa = q.plan.final_act;
                                const int want_rel = fa == fop.dst ? DAD_SEAM_BUF_DST : fa == fop.rdst ? DAD_SEAM_BUF_RDST : DAD_SEAM_BUF_APART;
                                CHECK(s.buffers == want_rel && seam_buffers_ok(q.plan, fop), "buffer relation %d, the plan's %d", s.buffers, want_rel);
                                if (want_rel == DAD_SEAM_BUF_APART) {
                                    const long rows = (long)fop.Lout * fop.M, a0 = q.plan.bufs[fa].offset;
                                    for (int id : {fop.dst, fop.rdst}) {
                                        const long b0 = q.plan.bufs[id].offset;
                                        CHECK(a0 + rows <= b0 || b0 + rows <= a0, "'apart' with overlapping floats");
                                    }
                                }
                            }
                            // the launch it replaces is the ragged first conv with the ride, in one K chunk
                            const ConvOp& op = q.plan.convs[f.launches[0].conv];
                            CHECK(g.ragged && g.fused && g.kc == 32 && g.split.kslices == 1 && op.cin0 == td && op.wtaps() == 6 && op.kc == 16, "first conv");
                            CHECK(op.cin_pad >= 16 && op.cin_pad % 16 == 0, "granule 0 exists");
                        }
                        m.step_seam = true; m.cc_enabled = true; m.fuse_residual = true; m.force_tile = -1; m.split_enabled = true;
                    }
                }
            }
    for (int why : {SEAM_TAKEN, SEAM_OPTION, SEAM_SMALL_BATCH, SEAM_PRECISION, SEAM_FORCED_TILE, SEAM_PROJECTION, SEAM_PADDED, SEAM_HORIZON,
                    SEAM_TRANSITION_DIM, SEAM_DIM, SEAM_FIRST_CONV, SEAM_NO_RIDE})
        CHECK(seen[why] > 0, "the sweep never met '%s'", seam_reason(why));
    std::set<std::string> names;
    for (int why = 0; why < SEAM_WHYS; ++why) names.insert(seam_reason(why));
    CHECK((int)names.size() == SEAM_WHYS, "every reason has a name of its own");
    printf("rule sweep: %d plans taken\n", taken);

    // tile 2 (128 x 64, eight float4 per thread: another GroupNorm reduction order) is refused
    {
        HostModel m;
        if (build(m, 6, 128, {1, 2}, 32)) {
            FwdPlan f;
            plan_forward(m, false, 1024, true, f);
            CHECK(f.launches[0].g.cfg == 2 && plan_seam(m, f, false).why == SEAM_TILE, "batch 1024: tile %d, '%s'", f.launches[0].g.cfg,
                  seam_reason(plan_seam(m, f, false).why));
            plan_forward(m, false, 256, true, f);
            const SeamPlan s = plan_seam(m, f, false);
            CHECK(s.taken() && !s.tile0 && s.units == 1 && s.grid == 256 && s.threads == 512, "the headline: '%s'", seam_reason(s.why));
        }
    }
    // the buffer condition: distinct buffers, or the very buffer read and written row for row; nothing else
    {
        Plan P;
        P.bufs = {{4096, 0}, {4096, 4096}, {4096, 8192}, {2048, 12288}};
        ConvOp op; op.M = 128; op.Lout = 32; op.cout = 128;
        auto ok = [&](int fin, int dst, int rdst) { P.final_act = fin; op.dst = dst; op.rdst = rdst; return seam_buffers_ok(P, op); };
        CHECK(ok(2, 0, 1), "three distinct buffers");
        CHECK(ok(0, 0, 1) && ok(1, 0, 1), "final_act is the buffer the conv (or the ride) writes: the same rows");
        CHECK(!ok(0, 0, 0) && !ok(2, 1, 1), "the conv and the ride write one buffer");
        CHECK(!ok(-1, 0, 1) && !ok(2, -1, 1) && !ok(2, 0, -1) && !ok(2, 0, 7), "a buffer that does not exist");
        P.bufs[1].offset = 2048;                            // two ids, overlapping floats
        CHECK(!ok(2, 0, 1) && !ok(1, 0, 2), "overlapping buffers");
        P.bufs[1].offset = 4096;
        CHECK(!ok(3, 0, 1), "final_act shorter than the tile rows");
        auto rel = [&](int fin, int dst, int rdst) { P.final_act = fin; op.dst = dst; op.rdst = rdst; return seam_buffer_relation(P, op); };
        CHECK(rel(2, 0, 1) == DAD_SEAM_BUF_APART && rel(0, 0, 1) == DAD_SEAM_BUF_DST && rel(1, 0, 1) == DAD_SEAM_BUF_RDST, "the three relations");
        CHECK(rel(0, 0, 0) == -1 && rel(3, 0, 1) == -1 && rel(2, 0, 7) == -1, "a refused plan has no relation");
    }
}

int main() {
    HostModel probe;
    for (int DIM : {32, 64, 128})
        for (int H : {8, 16, 32})
            for (int td : {1, 3, 6, 8, 9, 15, 16})
                for (int t0 = 0; t0 < 2; ++t0) {
                    if (!t0 && DIM < 64) continue;
                    for (int nvalid = 1; nvalid <= 32 / H; ++nvalid)
                        for (int sh = 0; sh < 2; ++sh) check_kernel(probe, DIM, H, td, t0 != 0, nvalid, sh != 0);
                }
    printf("%ld fragment reads checked\n", g_reads);
    check_rule();
    if (g_failures) { printf("%d failures\n", g_failures); return 1; }
    printf("seam host logic ok\n");
    return 0;
}
