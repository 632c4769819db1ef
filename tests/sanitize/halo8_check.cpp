// halo8_check.cpp — the host side of csrc/conv_halo8.hpp (the halo-skipping kernel of 8-position 5-tap convs), checked
// without HIP under -fsanitize=address,undefined.  The kernel's address arithmetic is repeated here from its lane map
// (conv_shapes.hpp halo8_*) and its constants, for both block tiles (32x64 SK4, 64x64 SK2), with and without the ride:
//   * find_xswz_pairs finds slot shifts, they keep a sample off its neighbour's real rows and inside the stage's slack;
//   * every ds_read_b64 of an operand fragment (both 32-lane groups, every wave, unit, block and stage) touches 64
//     distinct banks;
//   * a simulated stage (halo zeroing + the staging stores, tagged) returns to every fragment read exactly the
//     (sample, position + tap - 2, channel) element of the conv, or a zero of the halo, and the weight of (tap, row,
//     channel): the A and B operands of one MFMA k index are the same channel;
//   * the products left out read halo rows only, every other (sample, position, tap, channel) product with a real row
//     is multiplied exactly once, and the accumulator -> exchange-tile row map is the A operand's;
//   * the planner takes the kernel exactly where DESIGN.md says (heuristic tile 0 / 1, no grid split-K, full-chip
//     regime, sampling plan), twelve launches on the PointMaze net at batch 256, none under a forced tile, with the
//     option off, below the regime, or in the training forward.
// Built and run by tests/test_halo8_host.py (CPU suite).
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

// the kernel's constants
constexpr int BN = 64, KC = 32, TAPS = 5, PAD = 2, L = 8, KP = KC + 4, KU = 8, G = KC / KU;
constexpr int SPT = BN / L, SEG = L + 2 * PAD, XROWS = SPT * SEG, XF = XROWS * KP + dad::kXSwzPad;

static long g_reads = 0;

static void check_kernel(int BM, int SK, bool RES, uint64_t xswz) {
    const int WTAPS = TAPS + (RES ? 1 : 0), GW = G / SK, TMW = BM / 32, WT = TMW * 2, NT = 64 * WT * SK, UW = WTAPS * GW;
    const int STAGE = XF + WTAPS * BM * KP;
    CHECK((size_t)2 * STAGE <= dad::conv_lds_floats(BM, BN, KC, TAPS, L, L, SK, false, WTAPS), "BM %d: the planner's LDS size holds two stages", BM);
    CHECK(STAGE % 4 == 0 && NT == 512, "BM %d: stage %d floats, %d threads", BM, STAGE, NT);
    auto shift = [&](int s) { return (int)((xswz >> (4 * s)) & 15) * 4; };
    // ---- the stage as the kernel fills it: -2 never written, -1 zero, else a tag
    std::vector<int> lds((size_t)STAGE, -2);
    for (int i = 0; i < SPT * 2 * PAD * (KP / 4); ++i) {            // halo zeroing
        const int hr = i / (KP / 4), c4 = i - hr * (KP / 4);
        const int s = hr / (2 * PAD), j = hr - s * (2 * PAD);
        const int row = s * SEG + (j < PAD ? j : L + j);
        const int at = row * KP + c4 * 4 + shift(s);
        CHECK(at >= 0 && at + 4 <= XF, "halo zeroing at %d outside the X stage", at);
        for (int e = 0; e < 4 && at + 4 <= XF; ++e) lds[(size_t)at + e] = -1;
    }
    const int KQ = KC / 4;
    for (int e = 0; e < BN * KQ; ++e) {                              // X items: one float4 per thread
        const int row = e / KQ, q = e - row * KQ, s = row >> 3, l = row & 7;
        const int at = (s * SEG + PAD + l) * KP + q * 4 + shift(s);
        CHECK(at >= 0 && at + 4 <= XF, "X store at %d outside the X stage", at);
        for (int c = 0; c < 4 && at + 4 <= XF; ++c) {
            CHECK(lds[(size_t)at + c] == -2, "X store of sample %d position %d lands on another row or a halo", s, l);
            lds[(size_t)at + c] = (s * L + l) * KC + q * 4 + c;
        }
    }
    for (int e = 0; e < WTAPS * BM * KQ; ++e) {                      // W items
        const int row = e / KQ, q = e - row * KQ;
        const int at = XF + row * KP + q * 4;
        CHECK(at + 4 <= STAGE, "W store at %d outside the stage", at);
        for (int c = 0; c < 4 && at + 4 <= STAGE; ++c) lds[(size_t)at + c] = row * KC + q * 4 + c;
    }
    // ---- every fragment read of every wave
    std::vector<int> done((size_t)SPT * L * TAPS * KC * (BM / 16), 0);   // (sample, position, tap, channel, M block) products
    std::vector<int> ride((size_t)SPT * L * KC * (BM / 16), 0);
    for (int wave = 0; wave < WT * SK; ++wave) {
        const int wt = wave % WT, ks = wave / WT, tn = wt / TMW, tm = wt % TMW;
        const int tap_first = dad::halo8_tap(tn, 0), tap_dir = tn ? -1 : 1;
        for (int u = 0; u < UW; ++u) {
            const int wtap = u / GW, gw = u - wtap * GW;
            const bool is_ride = RES && wtap == TAPS;
            const int tap_a = is_ride ? PAD : tap_first + wtap * tap_dir, tap_b = is_ride ? TAPS : tap_first + wtap * tap_dir;
            CHECK(is_ride || tap_a == dad::halo8_tap(tn, wtap), "tap index %d of wave tile %d", wtap, tn);
            for (int nb = 0; nb < 2; ++nb) {
                const bool skipped = wtap == 0 && nb == 0;
                const int q = dad::halo8_block(tn, nb);
                int addr_a[64], addr_b[64];
                bool any_real = false;
                for (int lane = 0; lane < 64; ++lane) {
                    const int i16 = lane & 15, kq = lane >> 4;
                    const int smp = dad::halo8_sample(i16), pos = dad::halo8_pos(i16, q);
                    const int koff = ks * (GW * KU) + 2 * kq;
                    addr_a[lane] = (smp * SEG + pos) * KP + shift(smp) + koff + tap_a * KP + gw * KU;
                    addr_b[lane] = XF + (tm * 32 + nb * 16 + i16) * KP + koff + tap_b * (BM * KP) + gw * KU;   // (nb doubles as mb here)
                    const int lsrc = pos + tap_a - PAD;                  // input position the conv reads
                    const bool real = lsrc >= 0 && lsrc < L;
                    any_real = any_real || real;
                    CHECK(addr_a[lane] >= 0 && addr_a[lane] + 2 <= XF && addr_a[lane] % 2 == 0, "A read at %d", addr_a[lane]);
                    CHECK(addr_b[lane] >= XF && addr_b[lane] + 2 <= STAGE && addr_b[lane] % 2 == 0, "B read at %d", addr_b[lane]);
                    if (addr_a[lane] < 0 || addr_a[lane] + 2 > XF || addr_b[lane] < XF || addr_b[lane] + 2 > STAGE) continue;
                    for (int e = 0; e < 2; ++e) {
                        const int ch = koff + gw * KU + e;               // chunk channel of k index kq, k-step e
                        const int want_a = real ? (smp * L + lsrc) * KC + ch : -1;
                        CHECK(lds[(size_t)addr_a[lane] + e] == want_a, "BM %d wave %d unit %d block %d lane %d: A holds %d, the conv reads %d", BM,
                              wave, u, nb, lane, lds[(size_t)addr_a[lane] + e], want_a);
                        CHECK(lds[(size_t)addr_b[lane] + e] == (tap_b * BM + tm * 32 + nb * 16 + i16) * KC + ch, "BM %d wave %d unit %d: B operand", BM, wave, u);
                        if (skipped || !real) continue;
                        for (int mb = 0; mb < 2; ++mb) {
                            const size_t at = ((((size_t)smp * L + pos) * TAPS + (is_ride ? 0 : tap_a)) * KC + ch) * (BM / 16) + tm * 2 + mb;
                            if (is_ride) ride[(((size_t)smp * L + pos) * KC + ch) * (BM / 16) + tm * 2 + mb]++;
                            else done[at]++;
                        }
                    }
                    ++g_reads;
                }
                CHECK(skipped ? !any_real : any_real, "wave tile %d tap index %d block %d: %s", tn, wtap, nb, skipped ? "skipped but reads a real row" : "reads halo rows only");
                // bank conflicts: a ds_read_b64 is served as lanes 0..31, then 32..63; 64 banks of 4 bytes
                if (xswz != 0)
                    for (int half = 0; half < 2; ++half) {
                        std::set<int> banks_a, banks_b;
                        for (int lane = half * 32; lane < half * 32 + 32; ++lane)
                            for (int e = 0; e < 2; ++e) { banks_a.insert((addr_a[lane] + e) & 63); banks_b.insert((addr_b[lane] + e) & 63); }
                        CHECK(skipped || banks_a.size() == 64, "BM %d wave %d unit %d block %d: A fragment read hits %zu banks", BM, wave, u, nb, banks_a.size());
                        CHECK(banks_b.size() == 64, "BM %d wave %d unit %d block %d: B fragment read hits %zu banks", BM, wave, u, nb, banks_b.size());
                    }
            }
        }
    }
    for (int s = 0; s < SPT; ++s)
        for (int l = 0; l < L; ++l)
            for (int t = 0; t < TAPS; ++t)
                for (int ch = 0; ch < KC; ++ch)
                    for (int mbk = 0; mbk < BM / 16; ++mbk) {
                        const bool real = l + t - PAD >= 0 && l + t - PAD < L;
                        const int n = done[((((size_t)s * L + l) * TAPS + t) * KC + ch) * (BM / 16) + mbk];
                        CHECK(n == (real ? 1 : 0), "BM %d: product (sample %d, position %d, tap %d, channel %d, M block %d) multiplied %d times", BM, s, l, t, ch, mbk, n);
                        if (t == 0 && RES) CHECK(ride[(((size_t)s * L + l) * KC + ch) * (BM / 16) + mbk] == 1, "BM %d: ride product", BM);
                    }
    // ---- accumulator -> exchange-tile row: register r of lane (i16, kq) is MFMA row 4 kq + r
    std::vector<int> hit((size_t)BN, 0);
    for (int tn = 0; tn < 2; ++tn)
        for (int nb = 0; nb < 2; ++nb)
            for (int kq = 0; kq < 4; ++kq)
                for (int r = 0; r < 4; ++r) {
                    const int i = 4 * kq + r;
                    const int row = dad::halo8_sample(i) * L + dad::halo8_pos(i, dad::halo8_block(tn, nb));
                    CHECK(row >= 0 && row < BN, "tile row %d", row);
                    if (row >= 0 && row < BN) hit[(size_t)row]++;
                }
    for (int n = 0; n < BN; ++n) CHECK(hit[(size_t)n] == 1, "tile row %d written by %d accumulator registers", n, hit[(size_t)n]);
}

static bool build(HostModel& m, int td, int dim, std::vector<int> mults, int horizon, bool training) {
    dad_cfg& c = m.cfg;
    c.transition_dim = td; c.dim = dim; c.time_dim = dim;
    c.n_levels = (int)mults.size();
    for (size_t i = 0; i < mults.size(); ++i) c.channels[i] = dim * mults[i];
    c.kernel_size = 5; c.horizon = horizon; c.n_timesteps = 20;
    c.predict_epsilon = c.clip_denoised = 1;
    m.training = training;
    int rc = check_cfg(&c);
    CHECK(rc == DAD_OK, "check_cfg: %s", g_err);
    if (rc != DAD_OK) return false;
    rc = build_plan(&m);
    CHECK(rc == DAD_OK, "build_plan: %s", g_err);
    return rc == DAD_OK;
}

static int count_halo8(const HostModel& m, bool train, int B, int* eligible = nullptr) {
    FwdPlan f;
    const int rc = plan_forward(m, train, B, false, f);
    CHECK(rc == DAD_OK, "plan_forward B=%d: %s", B, g_err);
    const Plan& plan = train ? m.tplan : m.plan;
    int n = 0;
    if (eligible) *eligible = 0;
    for (const FwdLaunch& l : f.launches) {
        const ConvOp& op = plan.convs[l.conv];
        if (eligible && op.kind == CONV_K5 && op.Lout == 8 && op.taps == 5) ++*eligible;
        if (!l.g.halo8) continue;
        ++n;
        CHECK(op.kind == CONV_K5 && op.taps == 5 && op.stride == 1 && op.Lin == 8 && op.Lout == 8 && !op.x3 && !op.bdir, "%s: not a layer of the kernel", op.name.c_str());
        CHECK((l.g.cfg == 0 || l.g.cfg == 1) && l.g.kc == 32 && !l.g.ragged && !l.g.padded && !l.g.windowed && l.g.split.kslices == 1 && l.g.gx == 1,
              "%s: tile %d kc %d kslices %d", op.name.c_str(), l.g.cfg, l.g.kc, l.g.split.kslices);
        CHECK((op.cin0 + op.cin1) % 32 == 0 && op.cin0 % 32 == 0 && op.cin_pad == op.cin0 + op.cin1, "%s: whole K chunks", op.name.c_str());
        CHECK((long)l.g.mtiles * l.g.ntiles_n >= kSplitMaxTiles, "%s: %d x %d tiles", op.name.c_str(), l.g.mtiles, l.g.ntiles_n);
        CHECK(l.g.threads == 512 && l.g.lds_bytes <= dad::kLdsBytes, "%s: %d threads, %zu bytes of LDS", op.name.c_str(), l.g.threads, l.g.lds_bytes);
        CHECK(l.g.fused == fused_at(m, op, l.g), "%s: the ride is fused_at's decision", op.name.c_str());
        CHECK(l.g.xswz8 == find_xswz_pairs(m, 8, 2, 9) && l.g.xswz8 != 0, "%s: slot shifts", op.name.c_str());
        CHECK(kernel_registered(l.g.cfg, op.taps, op.stride, false, false, false, l.g.fused), "%s: the conv-GEMM twin (option off) exists", op.name.c_str());
    }
    return n;
}

int main() {
    HostModel probe;
    const uint64_t xswz = find_xswz_pairs(probe, L, PAD, KP / 4);
    CHECK(xswz != 0, "no conflict-free slot shifts for L = 8, KP = %d", KP);
    CHECK(find_xswz_pairs(probe, L, PAD, KP / 4) == xswz, "the memo returns another value");
    CHECK(find_xswz_pairs(probe, 16, PAD, KP / 4) == 0, "shifts for a length the kernel does not exist for");
    for (int s = 0; s + 1 < SPT; ++s) {
        const int d0 = (int)((xswz >> (4 * s)) & 15), d1 = (int)((xswz >> (4 * (s + 1))) & 15);
        CHECK(d0 - d1 <= PAD * (KP / 4), "shift pushes sample %d onto its neighbour", s);
    }
    CHECK(15 * 4 <= dad::kXSwzPad && (xswz >> 32) == 0, "slot shift slack");
    printf("slot shifts (L = 8, KP = %d): %08llx\n", KP, (unsigned long long)xswz);
    for (uint64_t sw : {xswz, (uint64_t)0})          // (shifts off: the same values, conflicts allowed)
        for (int res = 0; res < 2; ++res) {
            check_kernel(32, 4, res != 0, sw);
            check_kernel(64, 2, res != 0, sw);
        }
    printf("%ld fragment reads checked\n", g_reads);

    {   // the planner: the tests' net (128 channels at 8 positions) ...
        HostModel m;
        if (build(m, 6, 32, {1, 2, 4}, 32, true)) {
            int eligible = 0;
            CHECK(count_halo8(m, false, 312, &eligible) == 0 && eligible > 0, "B=312: 156 tiles are below the regime");
            // 40 N tiles: the eight launches with 128 output channels (4 M tiles of tile 0) reach 160 tiles, the four
            // with 64 output channels (decoder) need 80 N tiles
            const int n = count_halo8(m, false, 313, &eligible);
            CHECK(n == 8 && eligible == 12, "B=313: %d of %d 8-position launches", n, eligible);
            CHECK(count_halo8(m, false, 323) == 8, "B=323 (a partly empty last tile)");
            CHECK(count_halo8(m, false, 632) == 8 && count_halo8(m, false, 633) == 12, "B=633: every 8-position launch");
            CHECK(count_halo8(m, true, 320) == 0, "the training forward keeps the conv-GEMM kernels");
            m.halo8_enabled = false;
            CHECK(count_halo8(m, false, 320) == 0, "option off");
            m.halo8_enabled = true;
            for (int force = 0; force < kNumTiles; ++force) { m.force_tile = force; CHECK(count_halo8(m, false, 320) == 0, "forced tile %d", force); }
            m.force_tile = -1; m.split_enabled = false;
            CHECK(count_halo8(m, false, 320) == 0 && count_halo8(m, false, 8) == 0, "split-K switched off (tile 99) pins the conv-GEMM kernels");
            m.split_enabled = true;
            m.precision = DAD_PREC_F16X3; decide_kernel_families(&m);
            CHECK(count_halo8(m, false, 320) == 0, "split-f16 arithmetic");
        }
    }
    {   // ... and the headline: PointMaze at batch 256, twelve launches (7 x 512 -> 512, 256 -> 512 and 1024 -> 256 with the ride,
        // 3 x 256 -> 256)
        HostModel m;
        if (build(m, 6, 128, {1, 2, 4}, 32, false)) {
            int eligible = 0, rides = 0, tile1 = 0;
            CHECK(count_halo8(m, false, 256, &eligible) == 12 && eligible == 12, "PointMaze B=256: %d of %d", count_halo8(m, false, 256), eligible);
            FwdPlan f;
            plan_forward(m, false, 256, false, f);
            for (const FwdLaunch& l : f.launches) if (l.g.halo8) { rides += l.g.fused; tile1 += l.g.cfg == 1; }
            CHECK(rides == 2 && tile1 == 8, "PointMaze B=256: %d rides, %d launches on tile 1", rides, tile1);
            CHECK(count_halo8(m, false, 1) == 0 && count_halo8(m, false, 64) == 0, "PointMaze: small batches");
        }
    }
    if (g_failures) { printf("%d failures\n", g_failures); return 1; }
    printf("halo8 host logic ok\n");
    return 0;
}
