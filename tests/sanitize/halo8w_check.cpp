// halo8w_check.cpp — the host side of conv_halo8w_f32 (csrc/conv_halo8.hpp: the register-weight form of the halo-skipping
// kernel), checked without HIP under -fsanitize=address,undefined.  The kernel's address arithmetic is repeated here from
// its wave map and constants, for both block tiles (32x64 SK4, 64x64 SK2), with and without the ride:
//   * the launch's LDS size (halo8w_lds_floats) holds two X stages and the epilogue's exchange tile;
//   * weights: over one chunk every (tap slot, channel, output row) of the tile is loaded by exactly one lane of exactly
//     one wave, from inside the packed image (weight_image.hpp: (((ci / 16) * wtaps + slot) * M + o) * 16 + ci % 16), and
//     the element a lane holds for k-step e of a unit is the channel its A fragment holds there;
//   * activations: every fragment read of the simulated stage (halo zeroing + the staging stores, tagged) returns the
//     (sample, position + tap - 2, channel) element of the conv or a zero of the halo, and touches 64 distinct banks;
//   * the products left out read halo rows only and every other (sample, position, tap, channel, M block) product with a
//     real row is multiplied exactly once; the ride's once;
//   * per output element, the (tap, channel) order of the products is conv_halo8_f32's, and so is the K slice;
//   * the accumulator -> exchange-tile map writes every (row, column) of the tile once per K slice;
//   * the planner: the form of a launch is the option's, its LDS size the form's.
// Built and run by tests/test_hip_halo8_wreg.py (CPU suite).
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
constexpr int BN = 64, KC = 32, TAPS = 5, PAD = 2, L = 8, KP = KC + 4, KU = 8, G = KC / KU, KG = 16, NSUB = KC / KG;
constexpr int SPT = BN / L, SEG = L + 2 * PAD, XROWS = SPT * SEG, STAGE = XROWS * KP + dad::kXSwzPad;

static long g_reads = 0, g_loads = 0;

struct Product { int tap, ch; };            // one product of an output element's sum: conv tap (5: the ride), chunk channel
static bool operator==(const Product& a, const Product& b) { return a.tap == b.tap && a.ch == b.ch; }

// The order conv_halo8_f32 adds the products of (block q, K slice ks, k-step e) in: its wave tile tn = q / 2 walks tap index
// t as conv tap halo8_tap(tn, t), groups inside, and leaves out its block 0 (q = 0 / q = 3) at tap index 0.
static std::vector<Product> old_order(int q, int ks, int e, int kq, int GW, int WTAPS) {
    std::vector<Product> out;
    const int tn = q / 2, nb = tn ? 3 - q : q;
    for (int u = 0; u < WTAPS * GW; ++u) {
        const int wtap = u / GW, gw = u - wtap * GW;
        if (wtap == 0 && nb == 0) continue;
        out.push_back({wtap == TAPS ? TAPS : dad::halo8_tap(tn, wtap), ks * (GW * KU) + 2 * kq + gw * KU + e});
    }
    return out;
}

static void check_kernel(int BM, int SK, bool RES, uint64_t xswz) {
    const int WTAPS = TAPS + (RES ? 1 : 0), GW = G / SK, TMW = BM / 16, NT = 64 * TMW * SK, UW = WTAPS * GW, NW = WTAPS * GW;
    const size_t lds = dad::halo8w_lds_floats(BM, SK);
    CHECK((size_t)2 * STAGE <= lds && (size_t)SK * BN * (BM + 4) + 32 <= lds && lds * sizeof(float) <= dad::kLdsBytes,
          "BM %d: %zu floats of LDS hold two stages and the exchange", BM, lds);
    CHECK(STAGE % 4 == 0 && NT == 512 && BN * (KC / 4) == NT, "BM %d: stage %d floats, %d threads, one X item each", BM, STAGE, NT);
    CHECK((NW + 1) / 2 < UW, "BM %d: the X item rolls after the weight loads, inside the chunk", BM);
    auto shift = [&](int s) { return (int)((xswz >> (4 * s)) & 15) * 4; };
    // ---- the X stage as the kernel fills it: -2 never written, -1 zero, else a tag
    std::vector<int> stage((size_t)STAGE, -2);
    for (int i = 0; i < SPT * 2 * PAD * (KP / 4); ++i) {            // halo zeroing
        const int hr = i / (KP / 4), c4 = i - hr * (KP / 4);
        const int s = hr / (2 * PAD), j = hr - s * (2 * PAD);
        const int row = s * SEG + (j < PAD ? j : L + j);
        const int at = row * KP + c4 * 4 + shift(s);
        CHECK(at >= 0 && at + 4 <= STAGE, "halo zeroing at %d outside the stage", at);
        for (int e = 0; e < 4 && at >= 0 && at + 4 <= STAGE; ++e) stage[(size_t)at + e] = -1;
    }
    const int KQ = KC / 4;
    for (int tid = 0; tid < NT; ++tid) {                             // the X item of every thread
        const int row = tid / KQ, q = tid - row * KQ, s = row >> 3, l = row & 7;
        const int at = (s * SEG + PAD + l) * KP + q * 4 + shift(s);
        CHECK(at >= 0 && at + 4 <= STAGE, "X store at %d outside the stage", at);
        for (int c = 0; c < 4 && at >= 0 && at + 4 <= STAGE; ++c) {
            CHECK(stage[(size_t)at + c] == -2, "X store of sample %d position %d lands on another row or a halo", s, l);
            stage[(size_t)at + c] = (s * L + l) * KC + q * 4 + c;
        }
    }
    // ---- the packed weight image of a layer with two M tiles and three chunks, tagged (slot, o, ci); the image of a
    // launch without the ride may still hold the ride's slot (p.wtaps is the image's)
    for (int image_taps = WTAPS; image_taps <= TAPS + 1; ++image_taps) {
        const int M = 2 * BM, nchunks = 3;
        const long n = (long)nchunks * NSUB * image_taps * M * KG;
        std::vector<long> image((size_t)n);
        for (int ci = 0; ci < nchunks * KC; ++ci)
            for (int slot = 0; slot < image_taps; ++slot)
                for (int o = 0; o < M; ++o)
                    image[(size_t)((((long)(ci / KG) * image_taps + slot) * M + o) * KG + ci % KG)] = ((long)slot * M + o) * 4096 + ci;
        const long w_chunk_stride = (long)NSUB * image_taps * M * KG;
        for (int mt = 0; mt < 2; ++mt)
            for (int chunk = 0; chunk < nchunks; ++chunk) {
                const int m0 = mt * BM;
                std::vector<int> loaded((size_t)WTAPS * KC * BM, 0);
                for (int wave = 0; wave < TMW * SK; ++wave) {
                    const int tm = wave % TMW, ks = wave / TMW;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int i16 = lane & 15, kq = lane >> 4;
                        const long wsrc = (long)(m0 + tm * 16 + i16) * KG + 2 * kq;
                        const int koff = ks * (GW * KU) + 2 * kq;    // the A side's
                        for (int k = 0; k < NW; ++k) {
                            const int slot = k / GW, gw = k - slot * GW;
                            const int c8 = (ks * GW + gw) * KU;
                            const long at = wsrc + chunk * w_chunk_stride + (long)(((c8 / KG) * image_taps + slot) * M) * KG + c8 % KG;
                            CHECK(at >= 0 && at + 2 <= n && at % 2 == 0, "BM %d wave %d lane %d item %d: weight load at %ld of %ld", BM, wave, lane, k, at, n);
                            if (at < 0 || at + 2 > n) continue;
                            for (int e = 0; e < 2; ++e) {
                                const int ch = koff + gw * KU + e;   // chunk channel of k index kq, k-step e: what frag_a holds
                                const int o = m0 + tm * 16 + i16;
                                CHECK(image[(size_t)at + e] == ((long)slot * M + o) * 4096 + chunk * KC + ch,
                                      "BM %d wave %d lane %d item %d k-step %d: holds %ld, the MFMA pairs it with slot %d row %d channel %d", BM, wave, lane, k, e,
                                      image[(size_t)at + e], slot, o, chunk * KC + ch);
                                loaded[((size_t)slot * KC + ch) * BM + tm * 16 + i16]++;
                            }
                            ++g_loads;
                        }
                    }
                }
                for (size_t i = 0; i < loaded.size(); ++i)
                    CHECK(loaded[i] == 1, "BM %d chunk %d: (slot %zu, channel %zu, row %zu) loaded %d times", BM, chunk, i / ((size_t)KC * BM), i / BM % KC, i % BM, loaded[i]);
            }
    }
    // ---- every fragment read and product of every wave
    std::vector<int> done((size_t)SPT * L * TAPS * KC * TMW, 0);     // (sample, position, tap, channel, M block) products
    std::vector<int> ride((size_t)SPT * L * KC * TMW, 0);
    for (int wave = 0; wave < TMW * SK; ++wave) {
        const int tm = wave % TMW, ks = wave / TMW;
        std::vector<Product> order[4][2][4];                         // [block][k-step][kq]
        for (int u = 0; u < UW; ++u) {
            const int wtap = u / GW, gw = u - wtap * GW;
            const bool is_ride = RES && wtap == TAPS;
            for (int q = 0; q < 4; ++q) {
                const bool skipped = wtap == 0 && (q == 0 || q == 3);
                const int tap = is_ride ? PAD : (q < 2 ? wtap : TAPS - 1 - wtap);       // frag_a's
                const int slot = is_ride ? TAPS : (q < 2 ? wtap : TAPS - 1 - wtap);     // wcur's index / GW of DAD8W_MFMA
                CHECK(is_ride || slot == tap, "the weight slot is the conv tap");
                int addr[64];
                bool any_real = false;
                for (int lane = 0; lane < 64; ++lane) {
                    const int i16 = lane & 15, kq = lane >> 4;
                    const int smp = dad::halo8_sample(i16), pos = dad::halo8_pos(i16, q);
                    const int koff = ks * (GW * KU) + 2 * kq;
                    const int afrag2 = ((smp * SEG + dad::halo8_pos(i16, 0)) * KP + shift(smp) + koff) >> 1;
                    addr[lane] = 2 * (afrag2 + q * KP + tap * (KP / 2) + gw * (KU / 2));
                    const int lsrc = pos + tap - PAD;                // input position the conv reads
                    const bool real = lsrc >= 0 && lsrc < L;
                    any_real = any_real || real;
                    CHECK(addr[lane] >= 0 && addr[lane] + 2 <= STAGE && addr[lane] % 2 == 0, "A read at %d", addr[lane]);
                    if (addr[lane] < 0 || addr[lane] + 2 > STAGE) continue;
                    for (int e = 0; e < 2; ++e) {
                        const int ch = koff + gw * KU + e;
                        const int want = real ? (smp * L + lsrc) * KC + ch : -1;
                        CHECK(stage[(size_t)addr[lane] + e] == want, "BM %d wave %d unit %d block %d lane %d: A holds %d, the conv reads %d", BM, wave, u, q,
                              lane, stage[(size_t)addr[lane] + e], want);
                        if (skipped) continue;
                        if (i16 == 0) order[q][e][kq].push_back({slot, ch});
                        if (!real) continue;
                        if (is_ride) ride[(((size_t)smp * L + pos) * KC + ch) * TMW + tm]++;
                        else done[((((size_t)smp * L + pos) * TAPS + tap) * KC + ch) * TMW + tm]++;
                    }
                    ++g_reads;
                }
                CHECK(skipped ? !any_real : any_real, "tap index %d block %d: %s", wtap, q, skipped ? "skipped but reads a real row" : "reads halo rows only");
                if (xswz != 0 && !skipped)                           // a ds_read_b64 is served as lanes 0..31, then 32..63; 64 banks of 4 bytes
                    for (int half = 0; half < 2; ++half) {
                        std::set<int> banks;
                        for (int lane = half * 32; lane < half * 32 + 32; ++lane)
                            for (int e = 0; e < 2; ++e) banks.insert((addr[lane] + e) & 63);
                        CHECK(banks.size() == 64, "BM %d wave %d unit %d block %d: A fragment read hits %zu banks", BM, wave, u, q, banks.size());
                    }
            }
        }
        for (int q = 0; q < 4; ++q)
            for (int e = 0; e < 2; ++e)
                for (int kq = 0; kq < 4; ++kq)
                    CHECK(order[q][e][kq] == old_order(q, ks, e, kq, GW, WTAPS), "BM %d wave %d block %d k-step %d: the products' order is not conv_halo8_f32's", BM, wave, q, e);
    }
    for (int s = 0; s < SPT; ++s)
        for (int l = 0; l < L; ++l)
            for (int t = 0; t < TAPS; ++t)
                for (int ch = 0; ch < KC; ++ch)
                    for (int mbk = 0; mbk < TMW; ++mbk) {
                        const bool real = l + t - PAD >= 0 && l + t - PAD < L;
                        const int n = done[((((size_t)s * L + l) * TAPS + t) * KC + ch) * TMW + mbk];
                        CHECK(n == (real ? 1 : 0), "BM %d: product (sample %d, position %d, tap %d, channel %d, M block %d) multiplied %d times", BM, s, l, t, ch, mbk, n);
                        if (t == 0) CHECK(ride[(((size_t)s * L + l) * KC + ch) * TMW + mbk] == (RES ? 1 : 0), "BM %d: ride product", BM);
                    }
    // ---- accumulator -> exchange tile: register r of lane (i16, kq) of block q is tile row (sample, position), column tm * 16 + i16
    const int ES = BM + 4;
    std::vector<int> hit((size_t)SK * BN * ES, 0);
    for (int wave = 0; wave < TMW * SK; ++wave)
        for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < 4; ++q)
                for (int r = 0; r < 4; ++r) {
                    const int tm = wave % TMW, ks = wave / TMW, i16 = lane & 15, kq = lane >> 4, i = 4 * kq + r;
                    const int row = dad::halo8_sample(i) * L + dad::halo8_pos(i, q), col = tm * 16 + i16;
                    const size_t at = (size_t)ks * BN * ES + (size_t)row * ES + col;
                    CHECK(row >= 0 && row < BN && col < BM && (at + 1) <= lds, "exchange element (%d, %d)", row, col);
                    if (at < hit.size()) hit[at]++;
                }
    for (int ks = 0; ks < SK; ++ks)
        for (int row = 0; row < BN; ++row)
            for (int col = 0; col < BM; ++col)
                CHECK(hit[(size_t)ks * BN * ES + (size_t)row * ES + col] == 1, "BM %d: exchange element (%d, %d, %d) written %d times", BM, ks, row, col,
                      hit[(size_t)ks * BN * ES + (size_t)row * ES + col]);
}

static bool build(HostModel& m, int td, int dim, std::vector<int> mults, int horizon) {
    dad_cfg& c = m.cfg;
    c.transition_dim = td; c.dim = dim; c.time_dim = dim;
    c.n_levels = (int)mults.size();
    for (size_t i = 0; i < mults.size(); ++i) c.channels[i] = dim * mults[i];
    c.kernel_size = 5; c.horizon = horizon; c.n_timesteps = 20;
    c.predict_epsilon = c.clip_denoised = 1;
    int rc = check_cfg(&c);
    CHECK(rc == DAD_OK, "check_cfg: %s", g_err);
    if (rc != DAD_OK) return false;
    rc = build_plan(&m);
    CHECK(rc == DAD_OK, "build_plan: %s", g_err);
    return rc == DAD_OK;
}

// halo8 launches of the plan at batch B, and how many of them take the register-weight form
static int count_forms(const HostModel& m, int B, int* wreg) {
    FwdPlan f;
    const int rc = plan_forward(m, false, B, false, f);
    CHECK(rc == DAD_OK, "plan_forward B=%d: %s", B, g_err);
    int n = 0;
    *wreg = 0;
    for (const FwdLaunch& l : f.launches) {
        CHECK(l.g.halo8 || !l.g.halo8w, "the register-weight form outside the halo8 launches");
        if (!l.g.halo8) continue;
        ++n;
        if (!l.g.halo8w) { CHECK(l.g.lds8w_bytes == 0, "an LDS size for a form not taken"); continue; }
        ++*wreg;
        const TileCfg& t = kTiles[l.g.cfg];
        CHECK(halo8_kernel_exists(l.g.cfg, l.g.fused) && t.BN == 64 && t.KC == 32 && l.g.threads == 64 * (t.BM / 16) * t.SK, "tile %d", l.g.cfg);
        CHECK(l.g.lds8w_bytes == dad::halo8w_lds_floats(t.BM, t.SK) * sizeof(float) && l.g.lds8w_bytes < l.g.lds_bytes, "tile %d: %zu bytes of LDS", l.g.cfg, l.g.lds8w_bytes);
    }
    return n;
}

int main() {
    HostModel probe;
    const uint64_t xswz = find_xswz_pairs(probe, L, PAD, KP / 4);
    CHECK(xswz != 0, "no conflict-free slot shifts for L = 8, KP = %d", KP);
    for (uint64_t sw : {xswz, (uint64_t)0})          // (shifts off: the same values, conflicts allowed)
        for (int res = 0; res < 2; ++res) {
            check_kernel(32, 4, res != 0, sw);
            check_kernel(64, 2, res != 0, sw);
        }
    printf("%ld fragment reads, %ld weight loads checked\n", g_reads, g_loads);

    HostModel m;                                     // PointMaze at batch 256: twelve launches, 8 on tile 1, 2 rides
    if (build(m, 6, 128, {1, 2, 4}, 32)) {
        int wreg = 0, expect = 0;
        FwdPlan f;
        plan_forward(m, false, 256, false, f);
        for (const FwdLaunch& l : f.launches) expect += l.g.halo8 && halo8w_faster(l.g.cfg, l.g.fused);
        CHECK(count_forms(m, 256, &wreg) == 12 && wreg == expect, "default: %d of 12 launches, halo8w_faster says %d", wreg, expect);
        m.halo8_wreg = 1;
        CHECK(count_forms(m, 256, &wreg) == 12 && wreg == 12, "option on: %d of 12", wreg);
        m.halo8_wreg = 0;
        CHECK(count_forms(m, 256, &wreg) == 12 && wreg == 0, "option off: %d of 12", wreg);
        m.halo8_wreg = 1; m.halo8_enabled = false;
        CHECK(count_forms(m, 256, &wreg) == 0 && wreg == 0, "without halo8 there is no form of it");
        m.halo8_enabled = true;
        CHECK(count_forms(m, 64, &wreg) == 0 && wreg == 0, "small batches");
    }
    if (g_failures) { printf("%d failures\n", g_failures); return 1; }
    printf("halo8w_check: ok\n");
    return 0;
}
