// long_horizon_check.cpp — the windowed-tile launches of layers longer than any tile (horizons 256 / 512 and
// horizons that pad up to them; csrc/host_plan.hpp kWinTiles, conv_gemm.hpp WIN, conv_gn_pass.hpp), checked on the
// host without HIP under -fsanitize=address,undefined against what the kernels assume:
//   * the windows of a launch cover every output row of every sample exactly once (through the XCD-order decode
//     when the launch uses it);
//   * every input row a window's taps read is staged, and staged rows come from the window's own sample only
//     (the halo never crosses into a neighbouring sample; outside the sample it is the conv's zero padding);
//   * the X stage the kernel sizes at compile time holds the staged rows, LDS fits, the GroupNorm pass holds the pair;
//   * grid split-K stays inside the ticket table and its slabs inside the workspace, for every batch the planner
//     admits, and batches beyond its guards are refused with a message.
// Built and run by tests/test_long_horizon_host.py (CPU suite).
#include <cstdio>
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
    int td, dim, horizon;
    std::vector<int> mults;
    int ks;
    int hreal;                    // dad_model_set_horizon (0: unpadded)
    std::vector<int> real;        // dad_model_set_group_channels (empty: unpadded)
};

static long g_windowed = 0, g_launches = 0;

// the kernel's decode of block (y, z) into (M tile, N tile), conv_gemm.hpp
static void decode(const LaunchGeom& g, long wg, long z, int& mt, int& nt) {
    if (g.xcd_gn > 0) {
        const int c = (int)(wg & 7), j = (int)(wg >> 3);
        const int im = c / g.xcd_gn, in = c - im * g.xcd_gn;
        mt = (im << g.xcd_mts) + (j & ((1 << g.xcd_mts) - 1));
        nt = in * g.xcd_ntn + (j >> g.xcd_mts);
    } else {
        mt = (int)wg;
        nt = (int)z;
    }
}

static void check_launch(HostModel& m, const ConvOp& op, int B, size_t ws) {
    LaunchGeom g;
    const int rc = plan_launch(m, op, B, g);
    const bool small_enough = (long)B * op.Lout * op.M < (1L << 31) && (long)B * op.Lin * (op.cin0 + op.cin1) < (1L << 31);
    if (rc != DAD_OK) {
        CHECK(g_err[0] != 0, "%s B=%d: refusal without a message", op.name.c_str(), B);
        // the heuristic refuses only through the size guards
        CHECK(!small_enough || tiles_n(op, kTiles[choose_tile(m, op, B) < 0 ? 0 : choose_tile(m, op, B)].BN, B) > 65535,
              "%s B=%d refused: %s", op.name.c_str(), B, g_err);
        return;
    }
    ++g_launches;
    const TileCfg& t = kTiles[g.cfg];
    CHECK(g.windowed == (op.Lout > t.BN), "%s: windowed flag", op.name.c_str());
    CHECK(g.windowed == windowed_layer(op), "%s: windowed only above %d positions (tile %d)", op.name.c_str(), kMaxTileBN, g.cfg);
    if (!g.windowed) return;
    ++g_windowed;
    CHECK(kWinTiles[g.cfg] && g.padded && !g.fused && !op.x3 && !op.bdir, "%s: windowed kernel family", op.name.c_str());
    CHECK(kernel_registered(g.cfg, op.taps, op.stride, op.x3, op.bdir, g.ragged, g.fused, g.padded, g.windowed),
          "%s: no windowed kernel", op.name.c_str());
    CHECK(op.Lout % t.BN == 0 && is_pow2(op.Lout), "%s: windows per sample", op.name.c_str());
    CHECK(g.lds_bytes <= dad::kLdsBytes, "%s: LDS %zu", op.name.c_str(), g.lds_bytes);
    const int S = op.Lin / op.Lout;                       // input rows per output row (2: down-sampling conv)
    const int pad = op.taps / 2;
    const int seg = t.BN * S + 2 * pad;                   // the kernel's SEG / XROWS
    CHECK(dad::conv_xrows(t.BN, op.Lin, op.Lout, op.taps) == seg, "%s: X stage rows", op.name.c_str());
    CHECK(op.kind == CONV_UP ? S == 1 : op.stride == S, "%s: stride %d vs Lin / Lout %d", op.name.c_str(), op.stride, S);
    if (!op.norm.empty())
        CHECK((long)(op.cout / 8) * op.Lout <= kGnPassMaxPair && (op.cout / 8) % 4 == 0, "%s: GroupNorm pass pair", op.name.c_str());

    // coverage: every (sample, output row) exactly once per M tile
    const int wsh = ilog2(op.Lout) - ilog2(t.BN);
    CHECK((1 << wsh) * t.BN == op.Lout, "%s: window shift", op.name.c_str());
    const long rows = (long)B * op.Lout;
    std::vector<unsigned char> hit((size_t)rows * g.mtiles, 0);
    const long blocks_yz = (long)g.gy * g.gz;
    for (long b = 0; b < blocks_yz; ++b) {
        int mt, nt;
        decode(g, g.xcd_gn > 0 ? b : b % g.gy, g.xcd_gn > 0 ? 0 : b / g.gy, mt, nt);
        if (mt >= g.mtiles || nt >= g.ntiles_n) { CHECK(false, "%s: tile out of range", op.name.c_str()); continue; }
        const int s0 = nt >> wsh, w0 = (nt & ((1 << wsh) - 1)) * t.BN;
        CHECK(s0 < B, "%s: window of sample %d beyond batch %d", op.name.c_str(), s0, B);
        if (s0 >= B) continue;
        for (int n = 0; n < t.BN; ++n) hit[((size_t)s0 * op.Lout + w0 + n) * g.mtiles + mt]++;
        // halo: every row a tap reads is staged, from this sample, at an input position inside [-pad, Lin + pad)
        const int phase_max = op.kind == CONV_UP ? 1 : 0;
        for (int n = 0; n < t.BN; n += t.BN - 1)
            for (int ph = 0; ph <= phase_max; ++ph)
                for (int j = 0; j < op.taps; ++j) {
                    const int srow = n * S + ph + j;                     // the kernel's arow + tap
                    CHECK(srow >= 0 && srow < seg, "%s: tap reads stage row %d of %d", op.name.c_str(), srow, seg);
                }
        for (int r = 0; r < seg; ++r) {
            const int l = w0 * S - pad + r;                              // input position of stage row r
            const bool loaded = l >= 0 && l < op.Lin;
            if (loaded) {
                const long grow = (long)s0 * op.Lin + l;
                CHECK(grow >= (long)s0 * op.Lin && grow < (long)(s0 + 1) * op.Lin, "%s: halo row outside its sample", op.name.c_str());
            } else {
                CHECK(l >= -pad && l < op.Lin + pad, "%s: zero halo row %d beyond the conv padding", op.name.c_str(), l);
            }
        }
    }
    for (size_t i = 0; i < hit.size(); ++i)
        if (hit[i] != 1) { CHECK(false, "%s B=%d: output row %zu written %d times", op.name.c_str(), B, i / g.mtiles, (int)hit[i]); break; }

    // staging items: X_PER_T float4 per thread cover the stage (the kernel's constexpr X_F4_MAX)
    const int kq = g.kc / 4;
    const int x_f4_max = (t.BN * (op.kind == CONV_DOWN ? 2 : op.stride) + 2 * pad) * kq;
    CHECK(x_f4_max == seg * kq, "%s: X stage items %d vs %d rows", op.name.c_str(), x_f4_max, seg);
    if (g.split.kslices > 1) {
        const long tiles = (long)g.mtiles * g.ntiles_n;
        CHECK(tiles <= kMaxSplitTiles, "%s: ticket table (%ld tiles)", op.name.c_str(), tiles);
        const size_t end = ((size_t)m.plan.floats_per_sample * B + (size_t)g.split.slab_floats) * sizeof(float);
        CHECK(end <= ws && g.split.slab_floats >= tiles * g.split.kslices * (long)t.BN * t.BM,
              "%s B=%d: split-K slabs beyond the workspace", op.name.c_str(), B);
    }
}

static void check_arch(const Arch& a) {
    HostModel m;
    dad_cfg& c = m.cfg;
    c.transition_dim = a.td; c.dim = a.dim; c.time_dim = a.dim;
    c.n_levels = (int)a.mults.size();
    for (size_t i = 0; i < a.mults.size(); ++i) c.channels[i] = a.dim * a.mults[i];
    c.kernel_size = a.ks; c.horizon = a.horizon; c.n_timesteps = 20;
    c.predict_epsilon = c.clip_denoised = 1;
    int rc = check_cfg(&c);
    CHECK(rc == DAD_OK, "%s: check_cfg: %s", a.name, g_err);
    if (rc != DAD_OK) return;
    for (size_t i = 0; i < a.real.size(); ++i) m.real_channels[i] = a.real[i];
    m.real_horizon = a.hreal;
    rc = build_plan(&m);
    CHECK(rc == DAD_OK, "%s: build_plan: %s", a.name, g_err);
    if (rc != DAD_OK) return;
    CHECK(training_refusal(m) == nullptr, "%s: fp32 training refused: %s", a.name, training_refusal(m));
    m.precision = DAD_PREC_F16X3;
    CHECK(training_refusal(m) != nullptr, "%s: split-f16 training must stay refused", a.name);
    m.precision = DAD_PREC_FP32;
    CHECK(!cc_plan(m, 1).ok, "%s: small-batch plan above 128 positions", a.name);
    const long before = g_windowed;
    for (int B : {1, 2, 3, 7, 32, 64, 100, 256, 257, 1024, 4096, 16384, 65536, 1 << 20})
        for (int force = -1; force < kNumTiles; force += (force < 2 ? 1 : kNumTiles)) {
            m.force_tile = force;
            for (int split = 0; split < 2; ++split) {
                m.split_enabled = split == 0;
                const size_t ws = workspace_bytes(m, B);
                for (const ConvOp& op : m.plan.convs) check_launch(m, op, B, ws);
            }
        }
    m.force_tile = -1; m.split_enabled = true;
    CHECK(g_windowed > before, "%s: no windowed launch", a.name);
    printf("  %-22s %3zu convs, windowed launches so far %ld\n", a.name, m.plan.convs.size(), g_windowed);
}

int main() {
    const std::vector<Arch> archs = {
        {"dim32_1-4-8_H256", 6, 32, 256, {1, 4, 8}, 5, 0, {}},
        {"dim32_1-4-8_H512", 6, 32, 512, {1, 4, 8}, 5, 0, {}},
        {"dim64_1-2-4_H256", 6, 64, 256, {1, 2, 4}, 5, 0, {}},
        {"dim128_1-2-4-8_H256", 6, 128, 256, {1, 2, 4, 8}, 5, 0, {}},
        {"pointmaze_H200", 6, 128, 256, {1, 2, 4}, 5, 200, {}},
        {"dim32_H384", 6, 32, 512, {1, 4, 8}, 5, 384, {}},
        {"dim32_k3_H256", 6, 32, 256, {1, 2, 4}, 3, 0, {}},
        {"dim32_k7_H512", 5, 32, 512, {1, 2, 4}, 7, 0, {}},
        {"dim96pad_H256", 6, 128, 256, {1, 2, 4}, 5, 0, {96, 192, 384}},
        {"td1_dim32_H256", 1, 32, 256, {1, 2}, 5, 0, {}},
    };
    for (const Arch& a : archs) check_arch(a);
    printf("%ld launches checked, %ld windowed\n", g_launches, g_windowed);
    if (g_failures) { printf("%d failures\n", g_failures); return 1; }
    printf("long horizon host logic ok\n");
    return 0;
}
