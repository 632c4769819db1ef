// host_plan.hpp — everything libdad_hip.so decides on the HOST before a kernel is launched:
// validation of the architecture, the launch plan of TemporalUnet.forward, workspace layout,
// weight packing (fp32 and split-f16 images), tile choice, grid-level split-K, the LDS slot
// shifts, the launch geometry of every conv-GEMM, the small-batch plan, and — per call — one description of
// everything a forward evaluation launches at a batch (FwdPlan, plan_forward) and of the backward pass (the list
// of steps of build_backward_plan with its per-batch geometry, train_scratch), and the workspace layout of the fused
// training objective behind both (objective_layout).  The entry points of dad_lib.hip
// build those two once per call, refuse before their first launch, and only replay them; the size queries and
// the plan reports (csrc/plan_report.hpp, which writes them down and decides nothing) read the same descriptions.
// Plain C++17, no HIP: dad_lib.hip includes it for the product,
// tests/sanitize/host_check.cpp compiles it host-only under -fsanitize=address,undefined.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iterator>
#include <map>
#include <string>
#include <vector>

#include "../../include/dad.h"
#include "conv_shapes.hpp"
#include "weight_image.hpp"

namespace dadhost {

inline thread_local char g_err[1024] = "";

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

enum ConvKind { CONV_K5 = 0, CONV_1X1 = 1, CONV_DOWN = 2, CONV_UP = 3 };

// One conv-GEMM launch of the plan.  Buffer ids index Plan::bufs; -1 = none,
// -2 = the external (B,H,td) trajectory tensor.
struct ConvOp {
    std::string name;        // weight key prefix, e.g. "downs.0.0.blocks.0.block.0"
    std::string norm;        // GroupNorm key prefix or ""
    ConvKind kind;
    int taps, stride;
    int cin0, cin1, cin_pad;
    int cout;                // real output channels
    int M;                   // GEMM rows (2*cout for CONV_UP)
    int Lin, Lout;           // GEMM per-sample lengths (CONV_UP: Lout == Lin, stores 2*Lin)
    int src0, src1, dst, res;
    int temb_off;            // offset into the per-t table, or -1
    int kc = 16;             // K chunk the weights are packed for (8 when C_out/8 == 256)
    bool x3 = false;         // weights packed as split-f16 images (dad_model_set_precision)
    bool bdir = false;       // wide tile: weight fragments go global -> registers
    // identity residual over a channel concat (decoder block whose 2*C_in equals C_out): the two
    // halves are copied side by side into the `res` buffer before this launch
    int cat0 = -1, cat1 = -1, cat_c0 = 0, cat_c1 = 0;
    // The 1x1 residual conv of a ResidualTemporalBlock reads exactly the rows the block's first
    // 5-tap conv stages (temporal_unet.py:117-121).  It exists in the plan as its own launch
    // (rider_of = index of that conv) and, where the kernel variant exists, ALSO as a sixth
    // "tap" inside that conv's weight image (rname/rdst; own accumulator, plain bias epilogue).
    // Which of the two runs is decided per batch (LaunchGeom::fused of the carrier): the ride needs the whole K in one
    // block, so batches small enough for grid-level split-K keep the separate launch.
    std::string rname;       // weight key prefix of the riding residual conv, or ""
    int rdst = -1;           // buffer the ride writes
    bool ride = false;       // weight image holds the sixth tap (decided at pack time)
    int rider_of = -1;       // this op is the stand-alone form of convs[rider_of]'s ride
    float c1 = 1.0f, c2 = 0.0f;   // x3: output scales 2^-s and 2^-(s+11)
    // training plan only (HostModel::tplan): where the forward keeps what the backward pass needs of a
    // GroupNorm'd conv — its pre-normalisation output (conv + bias) and the (mean, rstd) of every
    // (sample, group) pair, [8][2] floats per sample
    int pre = -1, stats = -1;
    bool net_padded = false; // the model has zero-padded rows or channels: every launch takes the PADDED kernels
    int gn_real = 0;         // > 0: channels per GroupNorm group that exist (the rest of the group is zero padding)
    int lreal = 0;           // > 0: GEMM output rows per sample that exist (dad_model_set_horizon: the rest are zero
                             //      padding: masked in the GroupNorm statistics, stored as zeros); 0: all of them
    int src_len = 0;         // > 0: rows per sample of the EXTERNAL src0 (the trajectory keeps its real horizon)
    int real_in = 0, real_out = 0;   // zero-padded horizon: real positions per sample of the input / output TENSOR (0: no padding)
    // device tensors (owned by the model)
    float* d_w = nullptr;
    float* d_bias = nullptr;
    float* d_gamma = nullptr;
    float* d_beta = nullptr;
    float* d_rbias = nullptr;
    double flops_per_sample = 0;
    int wtaps() const { return taps + (ride ? 1 : 0); }      // tap slots of the packed image
    bool padded() const { return gn_real > 0 || lreal > 0 || src_len > 0; }   // runs the PADDED kernel instantiations
};

struct Buf {
    long per_sample;   // floats per batch row
    long offset;       // floats per batch row, from workspace start
};

struct Plan {
    std::vector<ConvOp> convs;
    std::vector<Buf> bufs;
    long floats_per_sample = 0;
    int final_act = -1;       // buffer holding final_conv[0] output
    int temb_width = 0;       // sum of C_out over residual blocks
};

constexpr int kMaxSplitTiles = 4096;
struct TileCfg { int BM, BN, SK, KC; };
// Block tile (BM channels x BN positions), SK-way intra-block split-K, K chunk.  Every
// configuration runs 8 waves per block except the last three.
constexpr int kNumTiles = 10;
constexpr TileCfg kTiles[kNumTiles] = {
    {32, 64, 4, 32},    // 0: few output tiles -> deepest split-K
    {64, 64, 2, 32},    // 1: the workhorse at batch 256
    {128, 64, 1, 16},   // 2: GroupNorm groups of 128 channels / plentiful tiles
    {256, 32, 1, 8},    // 3: GroupNorm groups of 256 channels (C = 2048)
    {64, 64, 1, 16},    // 4: plentiful tiles, 4 waves
    {32, 64, 2, 16},    // 5: 4 waves, small LDS: several independent blocks per CU
    {32, 64, 1, 16},    // 6: 2 waves
    {64, 64, 2, 16},    // 7: as 1 with the shallower K chunk (two blocks per CU fit)
    {32, 128, 2, 32},   // 8: layers of 128 positions (horizon 128, QUICKSTART.md:82): one sample per tile
    {64, 128, 1, 16},   // 9: the same with 64-channel tiles (GroupNorm groups of 64 channels)
};
constexpr int kMaxTileBN = 128;   // the longest layer a whole-sample tile holds
// Layers longer than kMaxTileBN (horizons 256 / 512 and the levels above 128 positions) run on WINDOWED tiles:
// BN consecutive positions of one sample per tile (conv_gemm.hpp, WIN), the GroupNorm tail as a second launch
// over whole (sample, group) pairs (conv_gn_pass.hpp).  Tiles with windowed instantiations:
constexpr bool kWinTiles[kNumTiles] = {true, true, true, false, false, false, false, false, false, false};
// Tiles with PADDED instantiations (zero-padded nets: the tiles choose_tile's heuristic picks):
constexpr bool kPaddedTiles[kNumTiles] = {true, true, true, true, true, false, false, false, true, true};
constexpr int kGnPassMaxPair = dad::GNP_THREADS * 4 * dad::kGnPassMaxNpt;   // elements of a (sample, group) pair the GroupNorm pass holds
inline bool windowed_layer(const ConvOp& op) { return op.Lout > kMaxTileBN; }
// N tiles of a launch: whole samples per tile, or Lout / BN windows per sample
inline long tiles_n(const ConvOp& op, int BN, int batch) {
    if (op.Lout > BN) return (long)batch * (op.Lout / BN);
    const int spt = BN / op.Lout;
    return (batch + spt - 1) / spt;
}

// 1x1 convs have one (tap, group) unit per 8 channels: a deep K chunk keeps enough MFMAs between
// barriers (128 channels; 64 for the 128-row tile, whose stage would not fit LDS twice).
// Split-f16 kernels consume 16 channels per unit: the chunk must give every split-K wave a unit.
// (128-position tiles: a 32-channel chunk — the deep one would not fit LDS twice next to 128 rows.)
constexpr int eff_kc(int cfg_kc, int bm, int taps, int sk = 1, bool x3 = false, bool bd = false, int bn = 64) {
    return bd                          ? 32          // wide tile, direct-B kernel (either arithmetic)
           : (taps == 1 && cfg_kc >= 16) ? (bn >= 128 ? 32 : bm >= 128 ? 64 : 128)
           : (x3 && cfg_kc < 16 * sk)  ? 16 * sk
                                       : cfg_kc;
}
// K chunk of tile `cfg` for a conv form: what the kernel is compiled with, and what the planner sizes LDS and the
// weight image with.
constexpr int tile_kc(int cfg, int taps, bool x3, bool bdir) {
    return eff_kc(kTiles[cfg].KC, kTiles[cfg].BM, taps, kTiles[cfg].SK, x3, bdir, kTiles[cfg].BN);
}

// ---- the backward pass as a list of steps (build_backward_plan), replayed by dad_unet_backward
// Operand of a step: a training-plan buffer's saved activation or its gradient (aliases resolved), or one of the
// pass's external tensors: the trajectory x, d loss / d out, the padded d x.
enum BwdSpace : int8_t { BSP_NONE, BSP_ACT, BSP_GRAD, BSP_X, BSP_DOUT, BSP_DX };
struct BwdRef { BwdSpace sp = BSP_NONE; int buf = -1; };
enum BwdKind : int8_t {
    BK_BIAS,     // per-sample partial sums of a bias gradient (row_partial_sums_kernel)
    BK_WGRAD,    // weight gradient (conv_wgrad)
    BK_DGRAD,    // data gradient: a conv-GEMM launch of BwdConv::op / bfinal
    BK_GN,       // GroupNorm + Mish backward, with the partial sums of d gamma, d beta, d bias
    BK_RESID,    // identity residual: the block's gradient into d x or a buffer
    BK_COLS,     // identity residual over a concat: one side's columns of the block's gradient
};
// How a step writes `out`: the first write of a gradient overwrites, later ones accumulate; a CONV_UP data gradient
// (its interleaving store has no residual operand) accumulates by staging through `tmp` and adding.
enum BwdWrite : int8_t { BW_SET, BW_ADD, BW_STAGE };
struct BwdStep {
    BwdKind kind;
    BwdWrite write = BW_SET;
    int conv = -1;          // forward conv (index into tplan.convs); -1: final_conv[1]
    int sub = 0;            // DGRAD: which data-gradient launch of that conv
    BwdRef in, out;         // the gradient read (WGRAD: the G operand) and the tensor written
    BwdRef z0, z1;          // WGRAD: the Z operands
    int slot = -1;          // WGRAD: gradient slot of the weight
    long part = 0;          // BIAS / GN: first partial-sum row, in units of B floats (GN: d gamma, d beta, d bias)
    long n = 0;             // RESID / DGRAD: floats per sample of `out`
    int rows = 0, C = 0;    // BIAS / COLS: rows per sample and channels (COLS: taken at column `off` of `ld`)
    int off = 0, ld = 0;
    int M = 0, C0 = 0, C1 = 0, taps = 0, stride = 0, pad = 0, Lg = 0, Lz = 0;   // WGRAD: the GEMM
    int nv = 0;             // GN: float4 per lane of gn_mish_bwd_wave_kernel<nv>; 0: gn_mish_bwd_kernel
};
// col_sums_many_kernel entry: gradient slot <- the sum over the batch of C partial-sum columns at `part`
struct BwdSum { int slot; long part; int C; };

// Host half of a model: what exists before any device allocation.
struct HostModel {
    dad_cfg cfg{};
    std::map<std::string, HostTensor> raw;
    std::map<std::string, std::vector<int64_t>> expected;     // key -> shape
    Plan plan;
    Plan tplan;                                                // the same launches with every tensor in a buffer of
                                                               // its own (nothing is overwritten before the backward
                                                               // pass has read it) + pre-activation / statistics buffers
    int precision = DAD_PREC_FP32;                             // dad_model_set_precision
    // tuning / test hooks (dad_debug_set_tile) — per model, nothing process-wide
    int force_tile = -1;
    bool split_enabled = true;
    bool fuse_residual = true;                                 // 1x1 residual conv rides in conv0
    bool xswz_enabled = true;
    bool xcd_order = true;
    int split_target = 256;
    bool cc_enabled = true;                                    // small batches take the consumer-combine kernels
    int cc_max_rows = 512;                                     //   up to this many batch * horizon rows
    int ccw_max_rows = 128;                                    //   the same for nets whose plan needs conv_ccw.hpp (wide layers)
    int ccw_min_blocks = 256;                                  //   blocks a wide layer keeps when its K slices are fattened
    int real_channels[DAD_MAX_LEVELS] = {0};                   // dad_model_set_group_channels: widths before padding (0: as cfg)
    int real_horizon = 0;                                      // dad_model_set_horizon: horizon before padding (0: as cfg)
    int wgrad_blocks = 256;                                    // blocks a weight-gradient launch aims for (tiles x batch splits)
    bool ccw_prefer16 = true;                                  //   two 16-row tiles instead of an LDS-short 32-row one
                                                               //   (measured crossover: batch 16 at H = 32)
    mutable std::map<std::array<int, 5>, uint64_t> xswz_cache; // find_xswz memo: the cache of a pure function, filled by const planning
    bool halo8_enabled = true;                                 // 8-position 5-tap layers at full-chip batches take conv_halo8.hpp
    mutable std::map<std::array<int, 3>, uint64_t> xswz8_cache; // find_xswz_pairs memo
    int halo8_wreg = -1;                                       //   ... as conv_halo8w_f32 (weights global -> register -> MFMA): 0 never,
                                                               //   1 every form, -1 the forms measured faster (halo8w_faster)
    bool step_seam = true;                                     // dad_sample_loop: posterior + next first conv as one launch (plan_seam)
    // ---- backward pass (dad_model_set_training): data-gradient launches + the layout of the gradients
    bool training = false;
    struct BwdConv {
        int n = 0;               // data-gradient launches of this forward conv (one per concat source)
        ConvOp op[2];
        int c_lo[2] = {0, 0};    // first input channel of the forward conv each one covers
        int c_n[2] = {0, 0};     // real channels (op.cout is c_n rounded up to 32)
    };
    std::vector<BwdConv> bconvs; // parallel to tplan.convs
    ConvOp bfinal;               // data gradient of final_conv[1] (1x1, transition_dim -> dim)
    struct GradSlot { std::string key; long offset, numel; };
    std::vector<GradSlot> grad_slots;        // flat gradient buffer: reference state_dict keys, torch layouts
    long grad_numel = 0;
    std::vector<GradSlot> time_grad_slots;   // the time-MLP gradients of the fused objective: a flat buffer of their own
    long time_grad_numel = 0;
    std::vector<BwdStep> bsteps;             // the backward pass in launch order
    std::vector<BwdSum> bsums;               // the column sums that end it, in order
    long bpart = 0;                          // partial-sum rows of the pass, in units of B floats
    bool bdx = false;                        // a gradient reaches the trajectory
    int bwd_rc = DAD_OK;                     // structural error of the pass, reported by dad_unet_backward
    std::string bwd_err;
    int max_cout = 0;                        // widest conv output (per-sample partial sums)
    int max_bwd_m = 0;                       // widest data-gradient launch (zero bias row)
};

inline int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }
inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// ----------------------------------------------------------------------------- validation
inline int check_cfg(const dad_cfg* cfg) {
    if (!cfg) return fail(DAD_E_INVALID, "null argument");
    if (cfg->kernel_size != 3 && cfg->kernel_size != 5 && cfg->kernel_size != 7)
        return fail(DAD_E_INVALID, "kernel_size %d unsupported (3, 5 or 7)", cfg->kernel_size);
    if (cfg->n_levels < 1 || cfg->n_levels > DAD_MAX_LEVELS)
        return fail(DAD_E_INVALID, "n_levels %d out of range", cfg->n_levels);
    if (cfg->transition_dim < 1 || cfg->dim < 4 || (cfg->dim & 1) || cfg->time_dim < 1)
        return fail(DAD_E_INVALID, "bad transition_dim/dim/time_dim");
    if (!is_pow2(cfg->horizon) || (cfg->horizon >> (cfg->n_levels - 1)) < 4)
        return fail(DAD_E_INVALID, "horizon %d must be a power of two with horizon / 2^(levels-1) >= 4",
                    cfg->horizon);
    if (cfg->n_timesteps < 1) return fail(DAD_E_INVALID, "n_timesteps must be positive");
    for (int i = 0; i < cfg->n_levels; ++i) {
        const int ch = cfg->channels[i];
        if (ch < 32 || ch % 32 != 0 || !is_pow2(ch / 8))
            return fail(DAD_E_INVALID, "level %d has %d channels: need a multiple of 32 with C/8 a power of two",
                        i, ch);
    }
    if (cfg->dim % 32 != 0) return fail(DAD_E_INVALID, "dim %d must be a multiple of 32", cfg->dim);
    return DAD_OK;
}

// ----------------------------------------------------------------------------- planning
struct Allocator {
    std::vector<Buf>& bufs;
    std::vector<bool> in_use;
    bool retain;                     // training plan: a buffer is never handed out twice
    explicit Allocator(std::vector<Buf>& b, bool keep = false) : bufs(b), retain(keep) {}
    int get(long per_sample) {
        int best = -1;
        for (size_t i = 0; i < bufs.size() && !retain; ++i)
            if (!in_use[i] && bufs[i].per_sample >= per_sample &&
                (best < 0 || bufs[i].per_sample < bufs[best].per_sample))
                best = (int)i;
        if (best < 0) {
            bufs.push_back({per_sample, 0});
            in_use.push_back(false);
            best = (int)bufs.size() - 1;
        }
        in_use[best] = true;
        return best;
    }
    void put(int id) { if (id >= 0) in_use[id] = false; }
};

inline void expect(HostModel* m, const std::string& key, std::vector<int64_t> shape) {
    m->expected[key] = std::move(shape);
}

// Which kernel family a conv belongs to — a function of the architecture and the precision only
// (so workspace sizes do not depend on whether weights have been loaded yet):
//   bdir  wide-group layers (op.kc == 8) use the direct-B kernel in either arithmetic: 16-channel
//         granules, whole 32-channel chunks, the net's k-tap stride-1 convs only (else the LDS-staged wide kernel)
//   ride  the weight image carries the block's 1x1 residual conv as a sixth tap (fp32, LDS-staged)
//   x3    split-f16 operands where the kernels exist for every tile this layer may get: 16-channel
//         granules, and for the strided / transposed convs (no general staging path) whole
//         64-channel chunks
inline void decide_kernel_families(HostModel* m) {
    // a zero-padded net (rows or channels) runs the PADDED instantiations everywhere: fp32, no ride
    bool padded_net = m->real_horizon > 0 && m->real_horizon != m->cfg.horizon;
    for (int i = 0; i < m->cfg.n_levels; ++i) padded_net = padded_net || (m->real_channels[i] > 0 && m->real_channels[i] != m->cfg.channels[i]);
    for (Plan* plan : {&m->plan, &m->tplan})
    for (ConvOp& op : plan->convs) {
        const int cin_all = op.cin0 + op.cin1;
        op.bdir = op.kc == 8 && op.kind == CONV_K5 &&
                  (op.cin0 % 32) == 0 && (cin_all % 32) == 0 && op.cin_pad == cin_all;
        // windowed layers (longer than any tile) run fp32 kernels only, without the ride: split-f16 nets mix them
        // with the split kernels of their shorter layers
        const bool win = windowed_layer(op);
        op.ride = !op.rname.empty() && !op.bdir && m->precision == DAD_PREC_FP32 && !padded_net && !win;
        op.x3 = !padded_net && !win && ((op.bdir && m->precision == DAD_PREC_F16X3) ||
                (m->precision == DAD_PREC_F16X3 && op.kc == 16 &&
                 ((op.kind == CONV_K5 && op.taps == 5) || op.kind == CONV_1X1 ||
                  ((op.kind == CONV_DOWN || op.kind == CONV_UP) && (op.cin0 & 63) == 0 && (cin_all & 63) == 0))));
        op.net_padded = padded_net;
    }
}

// Emits the launch plan of TemporalUnet.forward (temporal_unet.py:199-241) including the
// reference's always-upsample decoder and unused level-0 skip.
inline int build_plan_into(HostModel* m, Plan& P, bool retain) {
    const dad_cfg& c = m->cfg;
    P = Plan();
    Allocator A(P.bufs, retain);
    const int k = c.kernel_size;
    const int tdm = c.time_dim;
    int temb_off = 0;

    int level_now = 0;               // level whose width the convs being emitted produce
    const bool rows_padded = m->real_horizon > 0 && m->real_horizon != c.horizon;
    int Lr_now = rows_padded ? m->real_horizon : c.horizon;      // real positions at the level being emitted
    auto conv = [&](const std::string& name, const std::string& norm, ConvKind kind, int src0,
                    int src1, int cin0, int cin1, int cout, int Lin, int dst, int res,
                    int toff) {
        ConvOp op;
        op.name = name; op.norm = norm; op.kind = kind;
        const int real = m->real_channels[level_now];
        if (!norm.empty() && real > 0 && real != cout) op.gn_real = real / 8;
        if (rows_padded) {
            // real rows per sample of the GEMM's output (the transposed conv's GEMM rows are its INPUT positions)
            const int lr_out = kind == CONV_DOWN ? Lr_now / 2 : Lr_now;
            const int lp_out = kind == CONV_DOWN ? Lin / 2 : Lin;
            if (lr_out != lp_out) op.lreal = lr_out;
            if (src0 == -2) op.src_len = Lr_now;
            op.real_in = Lr_now;
            op.real_out = kind == CONV_DOWN ? Lr_now / 2 : kind == CONV_UP ? 2 * Lr_now : Lr_now;
        }
        op.cin0 = cin0; op.cin1 = cin1;
        op.kc = (!norm.empty() && cout / 8 >= 256) ? 8 : 16;
        const int padto = op.kc == 8 ? 8 : (kind == CONV_1X1 ? 128 : 64);   // deepest K chunk of its kernels
        op.cin_pad = (cin0 + cin1 + padto - 1) / padto * padto;
        op.cout = cout; op.src0 = src0; op.src1 = src1; op.dst = dst; op.res = res;
        op.temb_off = toff; op.Lin = Lin;
        const int cin = cin0 + cin1;
        switch (kind) {
            case CONV_K5: op.taps = k; op.stride = 1; op.M = cout; op.Lout = Lin;
                expect(m, name + ".weight", {cout, cin, k});
                op.flops_per_sample = 2.0 * cout * cin * k * Lin; break;
            case CONV_1X1: op.taps = 1; op.stride = 1; op.M = cout; op.Lout = Lin;
                expect(m, name + ".weight", {cout, cin, 1});
                op.flops_per_sample = 2.0 * cout * cin * Lin; break;
            case CONV_DOWN: op.taps = 3; op.stride = 2; op.M = cout; op.Lout = Lin / 2;
                expect(m, name + ".weight", {cout, cin, 3});
                op.flops_per_sample = 2.0 * cout * cin * 3 * (Lin / 2); break;
            case CONV_UP: op.taps = 2; op.stride = 1; op.M = 2 * cout; op.Lout = Lin;
                expect(m, name + ".weight", {cin, cout, 4});
                op.flops_per_sample = 2.0 * cout * cin * 4 * Lin; break;   // algorithmic
        }
        expect(m, name + ".bias", {cout});
        if (!norm.empty()) {
            expect(m, norm + ".weight", {cout});
            expect(m, norm + ".bias", {cout});
            if (retain) { op.pre = A.get((long)cout * op.Lout); op.stats = A.get(16); }
        }
        P.convs.push_back(op);
    };

    // widths before zero-padding (dad_model_set_group_channels): which blocks have a residual conv is a property of
    // the REAL widths (40 / 80 / 120 channels run as 64 / 128 / 128: the 80 -> 120 block keeps its 1x1 conv)
    auto realw = [&](int level) { return m->real_channels[level] > 0 ? m->real_channels[level] : c.channels[level]; };
    bool padded_net = false;
    for (int i = 0; i < c.n_levels; ++i) padded_net = padded_net || realw(i) != c.channels[i];
    const char* plan_error = nullptr;
    auto res_block = [&](const std::string& base, int in0, int in1, int cin0, int cin1, int cout,
                         int L, int rcin, int rcout) -> int {
        const int cin = padded_net ? (rcin == rcout ? cout : cout + 1) : cin0 + cin1;   // only compared with cout below
        const int toff = temb_off;
        temb_off += cout;
        expect(m, base + ".time_mlp.1.weight", {cout, tdm});
        expect(m, base + ".time_mlp.1.bias", {cout});
        const int a0 = A.get((long)cout * L);
        conv(base + ".blocks.0.block.0", base + ".blocks.0.block.1", CONV_K5, in0, in1, cin0, cin1,
             cout, L, a0, -1, toff);
        int res = -1;
        const bool cat_identity = cin == cout && in1 >= 0;   // nn.Identity over torch.cat([x, skip])
        if (cat_identity && padded_net)
            plan_error = "an identity residual over a channel concat (shrinking dim_mults) with zero-padded GroupNorm groups";
        if (cin != cout) {
            res = A.get((long)cout * L);
            const int c0 = (int)P.convs.size() - 1;
            conv(base + ".residual_conv", "", CONV_1X1, in0, in1, cin0, cin1, cout, L, res, -1, -1);
            if (P.convs[c0].kc == 16) {          // LDS-staged weights: a sixth tap can ride
                P.convs[c0].rname = base + ".residual_conv";
                P.convs[c0].rdst = res;
                P.convs.back().rider_of = c0;
            }
        } else if (cat_identity) {
            res = A.get((long)cout * L);
        }
        const int out = A.get((long)cout * L);
        conv(base + ".blocks.1.block.0", base + ".blocks.1.block.1", CONV_K5, a0, -1, cout, 0,
             cout, L, out, res >= 0 ? res : in0, -1);
        if (cat_identity) {
            ConvOp& last = P.convs.back();
            last.cat0 = in0; last.cat1 = in1; last.cat_c0 = cin0; last.cat_c1 = cin1;
        }
        A.put(a0);
        A.put(res);
        return out;
    };

    expect(m, "time_mlp.1.weight", {4 * tdm, c.dim});
    expect(m, "time_mlp.1.bias", {4 * tdm});
    expect(m, "time_mlp.3.weight", {tdm, 4 * tdm});
    expect(m, "time_mlp.3.bias", {tdm});

    const int nl = c.n_levels;
    int L = c.horizon;
    int x = -2, cx = c.transition_dim;
    std::vector<int> skips, skip_ch;
    for (int i = 0; i < nl; ++i) {
        const int co = c.channels[i];
        level_now = i;
        const std::string b = "downs." + std::to_string(i);
        const int h1 = res_block(b + ".0", x, -1, cx, 0, co, L, i == 0 ? c.transition_dim : realw(i - 1), realw(i));
        if (x >= 0) A.put(x);
        const int h2 = res_block(b + ".1", h1, -1, co, 0, co, L, realw(i), realw(i));
        A.put(h1);
        skips.push_back(h2);
        skip_ch.push_back(co);
        if (i < nl - 1) {
            const int d = A.get((long)co * (L / 2));
            conv(b + ".2.conv", "", CONV_DOWN, h2, -1, co, 0, co, L, d, -1, -1);
            L /= 2;
            Lr_now /= 2;
            x = d;
            if (i == 0) A.put(h2);   // level-0 skip is pushed but never popped (F8)
        } else {
            x = h2;
        }
        cx = co;
    }
    const int cm = c.channels[nl - 1];
    level_now = nl - 1;
    const int m1 = res_block("mid_block1", x, -1, cm, 0, cm, L, realw(nl - 1), realw(nl - 1));
    const int m2 = res_block("mid_block2", m1, -1, cm, 0, cm, L, realw(nl - 1), realw(nl - 1));
    A.put(m1);
    x = m2;
    cx = cm;
    for (int j = 0; j < nl - 1; ++j) {
        const int lvl = nl - 1 - j;                 // level whose skip is popped
        const int skip = skips[lvl];
        const int cs = skip_ch[lvl];
        const int co = c.channels[lvl - 1];
        level_now = lvl - 1;
        const std::string b = "ups." + std::to_string(j);
        const int u1 = res_block(b + ".0", x, skip, cx, cs, co, L, (j == 0 ? realw(nl - 1) : realw(lvl)) + realw(lvl), realw(lvl - 1));
        A.put(x);
        A.put(skip);
        const int u2 = res_block(b + ".1", u1, -1, co, 0, co, L, realw(lvl - 1), realw(lvl - 1));
        A.put(u1);
        const int up = A.get((long)co * (2 * L));
        conv(b + ".2.conv", "", CONV_UP, u2, -1, co, 0, co, L, up, -1, -1);
        A.put(u2);
        L *= 2;
        Lr_now *= 2;
        x = up;
        cx = co;
    }
    if (rows_padded)
        for (const ConvOp& op : P.convs)
            if (op.res == -2) plan_error = "transition_dim == dim (the first block's residual is the trajectory itself) with a zero-padded horizon";
    if (plan_error != nullptr) return fail(DAD_E_INVALID, "%s", plan_error);
    if (cx != c.dim)
        return fail(DAD_E_INVALID, "final_conv expects %d channels but the decoder ends with %d "
                    "(reference requires dim_mults[0] == 1)", c.dim, cx);
    const int f = A.get((long)c.dim * L);
    level_now = 0;
    conv("final_conv.0.block.0", "final_conv.0.block.1", CONV_K5, x, -1, cx, 0, c.dim, L, f, -1, -1);
    P.final_act = f;
    expect(m, "final_conv.1.weight", {c.transition_dim, c.dim, 1});
    expect(m, "final_conv.1.bias", {c.transition_dim});
    P.temb_width = temb_off;

    long off = 0;
    for (auto& b : P.bufs) {
        b.offset = off;
        off += (b.per_sample + 3) / 4 * 4;
    }
    P.floats_per_sample = off;
    return DAD_OK;
}
// ------------------------------------------------------------------------- backward plan
// The data gradient of every conv is itself a conv on the forward kernels, with its own weight image:
//   Conv1d k (stride 1)          dX[ci,i] = sum_co sum_k' W[co,ci,K-1-k'] dY[co, i - K/2 + k']     same kind, transposed + flipped
//   Downsample1d (k3, s2, p1)    dX[ci, 2j-1+k] += W[co,ci,k] dY[co,j]   = a ConvTranspose1d(k4,s2,p1) whose 4th tap is zero
//   Upsample1d (convT k4,s2,p1)  dX[ci,i] = sum_co sum_kk Wt[ci,co,kk] dY[co, 2i-1+kk]            = a 5-tap stride-2 conv (pad 2) whose first tap is zero
// (/root/reference/m_diffuser/models/temporal_unet.py:35-76; autograd's conv backward, restated.)
inline int round_up(int v, int to) { return (v + to - 1) / to * to; }
inline ConvOp make_bwd_op(const ConvOp& f, const char* tag, ConvKind kind, int taps, int stride, int cin, int c_n,
                          int Lin, int Lout) {
    ConvOp b;
    b.name = f.name + tag;
    b.kind = kind; b.taps = taps; b.stride = stride;
    b.cin0 = cin; b.cin1 = 0;
    b.kc = 16;
    b.cin_pad = round_up(cin, kind == CONV_1X1 ? 128 : 64);
    b.cout = round_up(c_n, 32);
    b.M = kind == CONV_UP ? 2 * b.cout : b.cout;
    b.Lin = Lin; b.Lout = Lout;
    b.src0 = b.src1 = b.dst = b.res = -1;
    b.temb_off = -1;
    b.flops_per_sample = 2.0 * b.cout * cin * (kind == CONV_UP ? 4 : taps) * Lout;
    return b;
}
inline int build_backward_plan(HostModel* m) {
    const Plan& P = m->tplan;
    const std::vector<ConvOp>& convs = P.convs;
    const dad_cfg& c = m->cfg;
    m->bconvs.assign(convs.size(), HostModel::BwdConv());
    m->grad_slots.clear(); m->grad_numel = 0;
    m->max_cout = c.dim; m->max_bwd_m = c.dim;
    auto slot = [&](const std::string& key, long numel) {
        m->grad_slots.push_back({key, m->grad_numel, numel});
        m->grad_numel += (numel + 3) / 4 * 4;
        return (int)m->grad_slots.size() - 1;
    };
    std::vector<int> wslot(convs.size()), bslot(convs.size()), gslot(convs.size(), -1);   // gslot + 1: GroupNorm bias
    for (size_t i = 0; i < convs.size(); ++i) {
        const ConvOp& f = convs[i];
        HostModel::BwdConv& b = m->bconvs[i];
        const int cin = f.cin0 + f.cin1;
        switch (f.kind) {
            case CONV_K5: case CONV_1X1:
                b.n = f.cin1 > 0 ? 2 : 1;
                for (int s = 0; s < b.n; ++s) {
                    b.c_lo[s] = s == 0 ? 0 : f.cin0;
                    b.c_n[s] = s == 0 ? f.cin0 : f.cin1;
                    b.op[s] = make_bwd_op(f, s == 0 ? ".dgrad0" : ".dgrad1", f.kind, f.taps, 1, f.cout, b.c_n[s], f.Lin, f.Lin);
                }
                wslot[i] = slot(f.name + ".weight", (long)f.cout * cin * f.taps);
                break;
            case CONV_DOWN:
                b.n = 1; b.c_lo[0] = 0; b.c_n[0] = cin;
                b.op[0] = make_bwd_op(f, ".dgrad0", CONV_UP, 2, 1, f.cout, cin, f.Lout, f.Lout);
                wslot[i] = slot(f.name + ".weight", (long)f.cout * cin * 3);
                break;
            case CONV_UP:
                b.n = 1; b.c_lo[0] = 0; b.c_n[0] = cin;
                b.op[0] = make_bwd_op(f, ".dgrad0", CONV_DOWN, 5, 2, f.cout, cin, 2 * f.Lin, f.Lin);
                wslot[i] = slot(f.name + ".weight", (long)cin * f.cout * 4);
                break;
        }
        // zero-padded horizon: the data gradient is zero-padded like every activation (its launches store zeros
        // behind the real rows: real GEMM rows = the forward conv's INPUT positions; the down-sampling conv's
        // data gradient is a transposed conv whose GEMM rows are the forward OUTPUT positions)
        for (int s = 0; s < b.n; ++s) {
            const int real_rows = f.kind == CONV_DOWN ? f.real_out : f.real_in;
            const int rows = f.kind == CONV_DOWN ? f.Lout : f.Lin;
            b.op[s].lreal = (real_rows > 0 && real_rows != rows) ? real_rows : 0;
            b.op[s].net_padded = f.net_padded;
        }
        bslot[i] = slot(f.name + ".bias", f.cout);
        if (!f.norm.empty()) { gslot[i] = slot(f.norm + ".weight", f.cout); slot(f.norm + ".bias", f.cout); }
        m->max_cout = std::max(m->max_cout, f.cout);
        for (int s = 0; s < b.n; ++s) m->max_bwd_m = std::max(m->max_bwd_m, b.op[s].M);
    }
    // final_conv[1]: 1x1, dim -> transition_dim; its data gradient is a 1x1 conv transition_dim -> dim
    {
        ConvOp f;
        f.name = "final_conv.1";
        m->bfinal = make_bwd_op(f, ".dgrad0", CONV_1X1, 1, 1, c.transition_dim, c.dim, c.horizon, c.horizon);
        if (m->real_horizon > 0 && m->real_horizon != c.horizon) { m->bfinal.lreal = m->real_horizon; m->bfinal.net_padded = true; }
    }
    const int fw = slot("final_conv.1.weight", (long)c.transition_dim * c.dim);
    const int fb = slot("final_conv.1.bias", c.transition_dim);

    // ---- the pass itself: final_conv[1], then the convs in reverse.  Gradients that meet in one tensor accumulate
    // in the order of this walk; the gradient of a 1x1 residual conv's output IS its block's gradient (an alias).
    std::vector<BwdStep>& S = m->bsteps;
    S.clear(); m->bsums.clear(); m->bpart = 0;
    m->bwd_rc = DAD_OK; m->bwd_err.clear();
    std::vector<int> alias(P.bufs.size(), -1), owner(P.bufs.size(), -1);
    std::vector<char> written(P.bufs.size(), 0);
    char dx = 0;
    for (size_t i = 0; i < convs.size(); ++i) owner[convs[i].dst] = (int)i;
    auto resolve = [&](int id) { while (alias[id] >= 0) id = alias[id]; return id; };
    auto grad = [&](int id) { return BwdRef{BSP_GRAD, resolve(id)}; };
    auto act = [&](int id) { return id == -2 ? BwdRef{BSP_X, -1} : id >= 0 ? BwdRef{BSP_ACT, id} : BwdRef{}; };
    auto write = [&](BwdStep& s, int id) {                 // s writes the gradient of buffer id (-2: the trajectory)
        char& w = id == -2 ? dx : written[resolve(id)];
        s.out = id == -2 ? BwdRef{BSP_DX, -1} : grad(id);
        s.write = w ? BW_ADD : BW_SET;
        w = 1;
    };
    auto part_take = [&](int C) { const long q = m->bpart; m->bpart += round_up(C, 4); return q; };
    auto bias = [&](BwdRef in, int rows, int C, int slot_) {
        BwdStep s{BK_BIAS};
        s.in = in; s.rows = rows; s.C = C; s.part = part_take(C);
        S.push_back(s);
        m->bsums.push_back({slot_, s.part, C});
    };
    auto wgrad = [&](BwdRef G, int M, BwdRef z0, int C0, BwdRef z1, int C1, int slot_, int taps, int stride, int pad,
                     int Lg, int Lz) {
        BwdStep s{BK_WGRAD};
        s.in = G; s.M = M; s.z0 = z0; s.C0 = C0; s.z1 = z1; s.C1 = C1; s.slot = slot_;
        s.taps = taps; s.stride = stride; s.pad = pad; s.Lg = Lg; s.Lz = Lz;
        S.push_back(s);
    };
    auto dgrad = [&](int conv, int sub, BwdRef dH, int target, long per_sample) {
        BwdStep s{BK_DGRAD};
        s.conv = conv; s.sub = sub; s.in = dH; s.n = per_sample;
        write(s, target);
        const ConvOp& op = conv < 0 ? m->bfinal : m->bconvs[conv].op[sub];
        if (op.kind == CONV_UP && s.write == BW_ADD) s.write = BW_STAGE;
        S.push_back(s);
    };

    const int H = c.horizon, td = c.transition_dim;
    const BwdRef dout{BSP_DOUT, -1};
    bias(dout, H, td, fb);
    wgrad(dout, td, act(P.final_act), c.dim, BwdRef{}, 0, fw, 1, 1, 0, H, H);
    dgrad(-1, 0, dout, P.final_act, (long)H * c.dim);
    for (int i = (int)convs.size() - 1; i >= 0; --i) {
        const ConvOp& f = convs[i];
        if (!written[resolve(f.dst)] && m->bwd_rc == DAD_OK) {
            m->bwd_rc = fail(DAD_E_STATE, "backward: no gradient reached the output of %s", f.name.c_str());
            m->bwd_err = g_err;
        }
        const BwdRef gout = grad(f.dst);
        const int out_rows = f.kind == CONV_UP ? 2 * f.Lout : f.Lout;      // rows per sample of the output
        BwdRef dH = gout;
        if (!f.norm.empty()) {
            auto resid = [&](int target) {
                BwdStep s{BK_RESID};
                s.in = gout; s.n = (long)out_rows * f.cout;
                write(s, target);
                S.push_back(s);
            };
            if (f.res == -2) {                            // identity residual of the trajectory itself (td == C)
                resid(-2);
            } else if (f.cat0 >= 0) {                     // identity residual over [cat0 | cat1]: each side takes its columns
                const int ids[2] = {f.cat0, f.cat1}, cs[2] = {f.cat_c0, f.cat_c1};
                for (int k = 0, off = 0; k < 2; off += cs[k], ++k) {
                    BwdStep s{BK_COLS};
                    s.in = gout; s.rows = out_rows; s.C = cs[k]; s.off = off; s.ld = f.cout;
                    write(s, ids[k]);
                    S.push_back(s);
                }
            } else if (f.res >= 0) {
                const int q = owner[f.res];
                if (q >= 0 && convs[q].kind == CONV_1X1 && convs[q].norm.empty()) alias[f.res] = resolve(f.dst);
                else resid(f.res);
            }
            BwdStep s{BK_GN};
            s.conv = i; s.in = gout; s.out = BwdRef{BSP_GRAD, f.pre};
            s.part = part_take(f.cout); part_take(f.cout); part_take(f.cout);
            // one wave per (sample, group) pair while the pair fits its registers, else one block per pair
            const int f4 = f.cout / 8 / 4 * f.Lout;
            s.nv = f4 <= 64 ? 1 : f4 <= 128 ? 2 : f4 <= 256 ? 4 : f4 <= 512 ? 8 : f4 <= 1024 ? 16 : 0;
            S.push_back(s);
            const long c4 = round_up(f.cout, 4);
            m->bsums.push_back({gslot[i], s.part, f.cout});
            m->bsums.push_back({gslot[i] + 1, s.part + c4, f.cout});
            m->bsums.push_back({bslot[i], s.part + 2 * c4, f.cout});
            dH = s.out;
        } else {
            bias(dH, out_rows, f.cout, bslot[i]);
        }
        switch (f.kind) {
            case CONV_K5: case CONV_1X1:
                wgrad(dH, f.cout, act(f.src0), f.cin0, act(f.src1), f.cin1, wslot[i], f.taps, 1, f.taps / 2, f.Lin, f.Lin); break;
            case CONV_DOWN:
                wgrad(dH, f.cout, act(f.src0), f.cin0, BwdRef{}, 0, wslot[i], 3, 2, 1, f.Lout, f.Lin); break;
            case CONV_UP:
                wgrad(act(f.src0), f.cin0, dH, f.cout, BwdRef{}, 0, wslot[i], 4, 2, 1, f.Lin, 2 * f.Lin); break;
        }
        const HostModel::BwdConv& b = m->bconvs[i];
        for (int k = 0; k < b.n; ++k) dgrad(i, k, dH, k == 0 ? f.src0 : f.src1, (long)f.Lin * b.c_n[k]);
    }
    m->bdx = dx != 0;
    return DAD_OK;
}
// Why a model cannot be trained on this engine, or nullptr.
// The ResidualTemporalBlocks in launch order: where each one's time projection sits in the (B, temb_width) rows the
// training forward reads (padded widths at their padded offsets).
struct TimeBlockRef { std::string base; int off, cout; };
inline std::vector<TimeBlockRef> time_block_list(const HostModel& m) {
    std::vector<TimeBlockRef> v;
    for (const ConvOp& op : m.tplan.convs)
        if (op.temb_off >= 0)
            v.push_back({op.name.substr(0, op.name.size() - std::strlen(".blocks.0.block.0")), op.temb_off, op.cout});
    return v;
}
// Gradient tensors of the time MLPs (dad_train_time_grad_info): time_mlp.1 / time_mlp.3, then every block's
// time_mlp.1 in launch order; torch layouts, each tensor at a multiple of four floats.
inline void build_time_grad_slots(HostModel* m) {
    m->time_grad_slots.clear(); m->time_grad_numel = 0;
    auto slot = [&](const std::string& key, long numel) {
        m->time_grad_slots.push_back({key, m->time_grad_numel, numel});
        m->time_grad_numel += (numel + 3) / 4 * 4;
    };
    const long tdm = m->cfg.time_dim;
    slot("time_mlp.1.weight", 4 * tdm * m->cfg.dim); slot("time_mlp.1.bias", 4 * tdm);
    slot("time_mlp.3.weight", tdm * 4 * tdm); slot("time_mlp.3.bias", tdm);
    for (const TimeBlockRef& b : time_block_list(*m)) {
        slot(b.base + ".time_mlp.1.weight", (long)b.cout * tdm);
        slot(b.base + ".time_mlp.1.bias", b.cout);
    }
}

inline const char* training_refusal(const HostModel& m) {
    if (m.precision != DAD_PREC_FP32) return "the backward pass exists for the fp32 arithmetic only";
    return nullptr;
}

inline bool tile_valid(const ConvOp& op, int cfg);
// An architecture some layer of which has no conv-GEMM tile is refused when the model is created, not at
// its first launch (validity of a tile does not depend on the batch).
inline int check_tiles(const HostModel& m) {
    for (const ConvOp& op : m.plan.convs) {
        bool any = false;
        for (int cfg = 0; cfg < kNumTiles && !any; ++cfg) any = tile_valid(op, cfg);
        if (!any)
            return fail(DAD_E_INVALID, "no tile configuration for %s (M=%d, C/8=%d, L=%d, %d taps)",
                        op.name.c_str(), op.M, op.cout / 8, op.Lout, op.taps);
    }
    return DAD_OK;
}
inline int build_plan(HostModel* m) {
    m->expected.clear();
    int rc = build_plan_into(m, m->plan, false);
    if (rc == DAD_OK) rc = build_plan_into(m, m->tplan, true);
    if (rc == DAD_OK) decide_kernel_families(m);
    if (rc == DAD_OK) rc = check_tiles(*m);
    if (rc == DAD_OK) rc = build_backward_plan(m);
    if (rc == DAD_OK) build_time_grad_slots(m);
    return rc;
}

// ------------------------------------------------------------------------------ packing
// Split-f16 image of a packed weight tensor (granules of 16 input channels):
//   [8 words: 16 hi halves | 8 words: 16 lo halves],  w * 2^s ~= hi + lo * 2^-11,
// s chosen per layer so the largest weight lands in [2^9, 2^10) and small ones stay normal halves.
// The kernel reads the words as the 32x32x16 f16 MFMA operand (conv_gemm.hpp, X3).
inline uint16_t f16_bits(float v) {
    const _Float16 h = (_Float16)v;       // round to nearest even
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}
inline int split_f16_image(std::vector<float>& packed) {
    float amax = 0.0f;
    for (float v : packed) amax = std::max(amax, std::fabs(v));
    int s = 0;
    if (amax > 0.0f && std::isfinite(amax)) {
        int e;
        std::frexp(amax, &e);             // amax = f * 2^e, f in [0.5, 1)
        s = 10 - e;                       // amax * 2^s in [2^9, 2^10)
    }
    s = std::max(-100, std::min(100, s));
    const float up = std::ldexp(1.0f, s);
    for (size_t g = 0; g + 16 <= packed.size(); g += 16) {
        uint16_t hi[16], lo[16];
        for (int j = 0; j < 16; ++j) {
            const float v = packed[g + j] * up;
            const _Float16 h = (_Float16)v;
            hi[j] = f16_bits(v);
            lo[j] = f16_bits((v - (float)h) * 2048.0f);
        }
        std::memcpy(&packed[g], hi, 32);
        std::memcpy(&packed[g + 8], lo, 32);
    }
    return s;
}

// Descriptors of the packed images (layouts: weight_image.hpp); dad_model_finalize and dad_model_refresh_weights
// both take them from here.
inline dad::ImageDesc image_desc(const ConvOp& op, int mode, int CO, int CI, int K, int c_lo = 0, int c_n = 0) {
    dad::ImageDesc p{};
    p.mode = mode;
    p.kg = op.bdir ? 16 : op.kc;                        // flags: decide_kernel_families
    p.wtaps = op.wtaps(); p.M = op.M;
    p.n = (long)op.cin_pad * p.wtaps * op.M;
    p.CO = CO; p.CI = CI; p.K = K; p.c_lo = c_lo; p.c_n = c_n;
    return p;
}
inline dad::ImageDesc fwd_image(const ConvOp& op) {        // the riding 1x1 conv, if any, is tap slot op.taps
    const int cin = op.cin0 + op.cin1;
    return op.kind == CONV_UP ? image_desc(op, dad::IMG_FWD_UP, op.cout, cin, 4) : image_desc(op, dad::IMG_FWD, op.cout, cin, op.taps);
}
// data-gradient launch k of forward conv f (see build_backward_plan)
inline dad::ImageDesc bwd_image(const ConvOp& f, const HostModel::BwdConv& b, int k) {
    const int mode = f.kind == CONV_DOWN ? dad::IMG_BWD_DOWN : f.kind == CONV_UP ? dad::IMG_BWD_UP : dad::IMG_BWD_CONV;
    return image_desc(b.op[k], mode, f.cout, f.cin0 + f.cin1, f.taps, b.c_lo[k], b.c_n[k]);
}
inline dad::ImageDesc bfinal_image(const HostModel& m) {
    return image_desc(m.bfinal, dad::IMG_BWD_FINAL, m.cfg.transition_dim, m.cfg.dim, 1);
}

// The device copies of the parameters, one entry each: a packed image or a plain copy.  dad_model_finalize packs
// and uploads them, dad_model_refresh_weights rebuilds them on the device from the same entries, and
// arena_bytes_needed counts them.
enum WeightTarget { WT_W, WT_BIAS, WT_RBIAS, WT_GAMMA, WT_BETA, WT_BWD_W, WT_BFINAL_W, WT_FINAL_W, WT_FINAL_B, WT_TIME };
struct WeightEntry {
    WeightTarget to;            // where the device pointer goes: d_w / d_bias / ... of plan.convs[conv],
    int conv, sub;              //   bconvs[conv].op[sub].d_w, bfinal.d_w, d_final_w / d_final_b or d_time[key]
    std::string key, key2;      // source tensors; key2: the riding 1x1 conv's weight (slot op.taps of the image)
    dad::ImageDesc img;         // img.n > 0: an image entry (its tensor pointers are filled where it is packed)
    long floats = 0;            // else a copy of `floats` floats, `reps` times over (2: the bias of both CONV_UP phases)
    int reps = 1;
    float* dev = nullptr;       // the device copy (dad_model_finalize)
    size_t size() const { return img.n > 0 ? (size_t)img.n : (size_t)floats * reps; }
};
inline std::vector<WeightEntry> weight_table(const HostModel& m) {
    std::vector<WeightEntry> t;
    auto copy = [&](WeightTarget to, int conv, const std::string& key, long floats, int reps = 1) {
        t.push_back({to, conv, 0, key, "", dad::ImageDesc{}, floats, reps});
    };
    for (const auto& kv : m.expected)        // time-MLP tensors: the per-timestep tables are derived from them
        if (kv.first.find("time_mlp.") != std::string::npos) {
            long n = 1;
            for (int64_t d : kv.second) n *= (long)d;
            copy(WT_TIME, -1, kv.first, n);
        }
    for (int i = 0; i < (int)m.plan.convs.size(); ++i) {
        const ConvOp& op = m.plan.convs[i];
        t.push_back({WT_W, i, 0, op.name + ".weight", op.ride ? op.rname + ".weight" : "", fwd_image(op)});
        for (int k = 0; m.training && k < m.bconvs[i].n; ++k)
            t.push_back({WT_BWD_W, i, k, op.name + ".weight", "", bwd_image(m.tplan.convs[i], m.bconvs[i], k)});
        copy(WT_BIAS, i, op.name + ".bias", op.cout, op.kind == CONV_UP ? 2 : 1);
        if (op.ride) copy(WT_RBIAS, i, op.rname + ".bias", op.cout);
        if (!op.norm.empty()) { copy(WT_GAMMA, i, op.norm + ".weight", op.cout); copy(WT_BETA, i, op.norm + ".bias", op.cout); }
    }
    copy(WT_FINAL_W, -1, "final_conv.1.weight", (long)m.cfg.transition_dim * m.cfg.dim);
    if (m.training) t.push_back({WT_BFINAL_W, -1, 0, "final_conv.1.weight", "", bfinal_image(m)});
    copy(WT_FINAL_B, -1, "final_conv.1.bias", m.cfg.transition_dim);
    return t;
}

// The host image of a descriptor: the elements in image order, so that none pays a division.
inline void pack_image(const dad::ImageDesc& p, float* out) {
    const long chunks = p.n / ((long)p.wtaps * p.M * p.kg);
    for (long c = 0; c < chunks; ++c)
        for (int slot = 0; slot < p.wtaps; ++slot)
            for (int o = 0; o < p.M; ++o)
                for (int j = 0; j < p.kg; ++j) *out++ = dad::image_value(p, (int)c * p.kg + j, slot, o);
}
// What dad_model_finalize uploads for an entry, from the host tensors.  A split-f16 conv's forward image is
// converted, and the conv receives its output scales.
inline int pack_entry(HostModel* m, const WeightEntry& e, std::vector<float>& out) {
    auto src = [&](const std::string& key) -> const float* {
        auto it = m->raw.find(key);
        return it == m->raw.end() ? nullptr : it->second.data.data();
    };
    const float* w = src(e.key);
    const float* ride = e.key2.empty() ? nullptr : src(e.key2);
    if (!w || (!e.key2.empty() && !ride)) return fail(DAD_E_KEY, "missing key '%s'", (w ? e.key2 : e.key).c_str());
    out.resize(e.size());
    if (e.img.n == 0) {
        for (int r = 0; r < e.reps; ++r) std::copy(w, w + e.floats, out.begin() + r * e.floats);
        return DAD_OK;
    }
    dad::ImageDesc p = e.img;
    p.w = w; p.ride = ride;
    pack_image(p, out.data());
    if (e.to == WT_W) {
        ConvOp& op = m->plan.convs[e.conv];
        op.c1 = 1.0f; op.c2 = 0.0f;
        if (op.x3) {
            const int sh = split_f16_image(out);
            op.c1 = std::ldexp(1.0f, -sh);
            op.c2 = std::ldexp(1.0f, -sh - 11);
        }
    }
    return DAD_OK;
}

// ------------------------------------------------------------------------- tile choice
// Hard constraints: the tile holds whole GroupNorm groups (BM % (C/8) == 0) and whole samples
// (BN % L == 0), BM divides the columns (each phase half for the transposed conv), the K chunk
// matches the packed weights.  Preference: enough blocks to cover the 256 CUs; when tiles are
// scarce, trade tile size for split-K depth.
inline bool tile_valid(const ConvOp& op, int cfg) {
    const TileCfg& t = kTiles[cfg];
    if (windowed_layer(op)) {
        // windowed route, only where no whole-sample tile exists: no GroupNorm constraint on the tile (the pass
        // after the conv owns whole pairs), fp32 LDS-staged kernels
        if (!kWinTiles[cfg] || op.x3 || op.bdir || op.kc != 16 || op.Lout % t.BN != 0) return false;
        if ((op.kind == CONV_UP ? op.M / 2 : op.M) % t.BM != 0) return false;
        if (!op.norm.empty() && (long)(op.cout / 8) * op.Lout > kGnPassMaxPair) return false;
        const int kc = tile_kc(cfg, op.taps, false, false);
        return dad::conv_lds_floats(t.BM, t.BN, kc, op.taps, op.Lin, op.Lout, t.SK, false, op.taps) * sizeof(float) <=
               dad::kLdsBytes;
    }
    if (op.net_padded && !kPaddedTiles[cfg]) return false;      // (PADDED kernels exist for the heuristic's tiles)
    const int Mrows = op.kind == CONV_UP ? op.M / 2 : op.M;
    const int cpg = op.norm.empty() ? 1 : op.cout / 8;
    if ((t.KC == 8) != (op.kc == 8)) return false;
    if (Mrows % t.BM != 0) return false;
    if (!op.norm.empty() && (t.BM % cpg != 0)) return false;
    if (t.BN % op.Lout != 0) return false;
    const int nthreads = 64 * (t.BM / 32) * (t.BN / 32) * t.SK;
    const int f4pl = t.BM * t.BN / 4 / nthreads;
    if (!op.norm.empty() && op.Lout * cpg / 4 < f4pl) return false;   // >= 1 lane per (group, sample)
    // the stage must fit LDS (the 128-position tiles with the 128-channel chunk of a 1x1 conv do not)
    const int kc = tile_kc(cfg, op.taps, op.x3, op.bdir);
    if (dad::conv_lds_floats(t.BM, t.BN, kc, op.taps, op.Lin, op.Lout, t.SK, op.bdir, op.taps) * sizeof(float) > dad::kLdsBytes)
        return false;
    return true;
}
inline int choose_tile(const HostModel& m, const ConvOp& op, int batch) {
    auto valid = [&](int cfg) { return tile_valid(op, cfg); };
    auto blocks = [&](int cfg) {
        const TileCfg& t = kTiles[cfg];
        return tiles_n(op, t.BN, batch) * (op.M / t.BM);
    };
    if (op.kc == 8) return valid(3) ? 3 : -1;
    if (m.force_tile >= 0 && m.force_tile < kNumTiles && valid(m.force_tile)) return m.force_tile;
    if (valid(2) && blocks(2) >= 512) return 2;          // plentiful work: big tile
    if (valid(1) && blocks(1) >= 224) return 1;
    if (valid(0)) return 0;
    if (valid(1)) return 1;
    if (valid(2)) return 2;
    if (valid(4)) return 4;
    if (valid(8)) return 8;              // 128 positions per sample
    if (valid(9)) return 9;
    return -1;
}

// Per-sample slot shifts of the X stage (conv_gemm.hpp, "Activation rows in LDS and bank
// conflicts").  Depth-first over the samples of a block tile: d(s) in [0, 16) such that in every
// 32-row wave tile both 16-lane groups of ds_read_b128 see 16 distinct slots, and no sample is
// pushed onto its neighbour's real rows (d(s) - d(s+1) <= pad * slots-per-row).  Returns 0 (plain
// layout — correct, just slower) when L >= 32, when there is no halo, or when nothing is found.
inline uint64_t find_xswz(const HostModel& m, int L, int stride, int pad, int kp4, int BN) {
    if (L >= 32 || pad == 0 || BN / L > 16) return 0;
    const std::array<int, 5> key{L, stride, pad, kp4, BN};
    auto it = m.xswz_cache.find(key);
    if (it != m.xswz_cache.end()) return it->second;
    static const int groups[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    const int S = BN / L, seg = L * stride + 2 * pad, per = 32 / L;
    std::vector<int> d(S, 0);
    // conflicts among the lanes whose samples are already placed (samples < upto)
    auto ok_prefix = [&](int upto) {
        for (int tn = 0; tn * per < upto; ++tn)
            for (const auto& g : groups) {
                unsigned seen = 0;
                for (int lane : g) {
                    const int n = tn * 32 + lane, sm = n / L, l = n % L;
                    if (sm >= upto) continue;
                    const unsigned bit = 1u << (((sm * seg + l * stride) * kp4 + d[sm]) & 15);
                    if (seen & bit) return false;
                    seen |= bit;
                }
            }
        return true;
    };
    long budget = 300000;                           // node budget: the search is a one-off per shape
    std::function<bool(int)> place = [&](int sm) -> bool {
        if (sm == S) return true;
        for (int v = 0; v < 16; ++v) {
            if (--budget < 0) return false;
            if (sm > 0 && d[sm - 1] - v > pad * kp4) continue;
            d[sm] = v;
            if (ok_prefix(sm + 1) && place(sm + 1)) return true;
        }
        d[sm] = 0;
        return false;
    };
    uint64_t packed = 0;
    if (place(0))
        for (int sm = 0; sm < S; ++sm) packed |= (uint64_t)d[sm] << (4 * sm);
    m.xswz_cache[key] = packed;
    return packed;
}

// The same for conv_halo8.hpp: a tile of eight 8-position samples read in position-pair-major column blocks with
// ds_read_b64 (lane map: conv_shapes.hpp halo8_*).  A ds_read_b64 is served in two groups of 32 lanes — 16 MFMA rows
// x two channel pairs kq — and is conflict-free when the group's 32 eight-byte slots are distinct mod 32.  Every
// block holds all eight samples, so one set of shifts serves every (wave tile, block, tap).  kp2: eight-byte slots
// per LDS row.  Returns 0 when nothing is found (plain layout: correct, slower).
inline bool xswz8_prefix_ok(const int* d, int upto, int seg, int kp2) {
    for (int q = 0; q < 4; ++q) {
        uint32_t seen = 0;
        for (int i = 0; i < 16; ++i) {
            const int sm = dad::halo8_sample(i);
            if (sm >= upto) continue;
            for (int kq = 0; kq < 2; ++kq) {
                const uint32_t bit = 1u << (((sm * seg + dad::halo8_pos(i, q)) * kp2 + 2 * d[sm] + kq) & 31);
                if (seen & bit) return false;
                seen |= bit;
            }
        }
    }
    return true;
}
inline uint64_t find_xswz_pairs(const HostModel& m, int L, int pad, int kp4) {
    if (L != 8 || pad == 0) return 0;
    const std::array<int, 3> key{L, pad, kp4};
    auto it = m.xswz8_cache.find(key);
    if (it != m.xswz8_cache.end()) return it->second;
    const int S = 8, seg = L + 2 * pad;
    int d[8] = {0};
    long budget = 300000;
    std::function<bool(int)> place = [&](int sm) -> bool {
        if (sm == S) return true;
        for (int v = 0; v < 16; ++v) {
            if (--budget < 0) return false;
            if (sm > 0 && d[sm - 1] - v > pad * kp4) continue;     // never onto the neighbour's real rows
            d[sm] = v;
            if (xswz8_prefix_ok(d, sm + 1, seg, 2 * kp4) && place(sm + 1)) return true;
        }
        d[sm] = 0;
        return false;
    };
    uint64_t packed = 0;
    if (place(0))
        for (int sm = 0; sm < S; ++sm) packed |= (uint64_t)d[sm] << (4 * sm);
    m.xswz8_cache[key] = packed;
    return packed;
}

// Grid-level split-K: when a layer has too few output tiles to cover the chip (small batches;
// the deepest levels of the wide nets), several blocks share a tile and split its K chunks.
constexpr int kSplitMaxTiles = 160;      // from this many output tiles on a launch is never split
struct SplitPlan { int kslices, chunks_per_slice; long slab_floats; };
inline SplitPlan plan_split(const HostModel& m, const ConvOp& op, int cfg, int batch) {
    const TileCfg& t = kTiles[cfg];
    const long tiles = tiles_n(op, t.BN, batch) * (op.M / t.BM);
    const int kc = tile_kc(cfg, op.taps, op.x3, op.bdir);
    const int nchunks = (op.cin0 + op.cin1 + kc - 1) / kc;      // chunks holding real channels
    SplitPlan sp{1, nchunks, 0};
    if (!m.split_enabled) return sp;
    if (tiles >= kSplitMaxTiles || nchunks < 2 || tiles > kMaxSplitTiles) return sp;
    // blocks = tiles * slices should not spill a few blocks into a second wave of the 256 CUs (24 tiles x
    // 11 slices = 264 blocks took 1.4x the time of 24 x 10): round the slice count DOWN while that still
    // splits, up only for tile counts above half the chip
    int want = tiles * 2 <= m.split_target ? (int)(m.split_target / tiles) : (int)((m.split_target + tiles - 1) / tiles);
    if (want > nchunks) want = nchunks;
    if (want < 2) return sp;
    sp.chunks_per_slice = (nchunks + want - 1) / want;
    sp.kslices = (nchunks + sp.chunks_per_slice - 1) / sp.chunks_per_slice;
    sp.slab_floats = tiles * sp.kslices * (long)t.BN * t.BM;
    return sp;
}

// ---------------------------------------------------------------------- launch geometry
// Everything a conv-GEMM launch needs besides pointers, decided on the host and checked here
// (operand shapes against what the kernel and its grid assume) before anything reaches the GPU.
struct LaunchGeom {
    int cfg = -1;            // index into kTiles
    int kc = 0;              // K chunk of the selected kernel instantiation
    bool ragged = false;     // general staging path (first layer, narrow nets)
    int threads = 0;
    size_t lds_bytes = 0;
    int ntiles_n = 0, mtiles = 0;
    unsigned gx = 1, gy = 1, gz = 1;
    int xcd_gn = 0, xcd_mts = 0, xcd_ntn = 0;
    bool fused = false;      // the residual conv rides in this launch
    bool padded = false;     // PADDED instantiation (zero-padded rows / channels; every windowed launch)
    bool windowed = false;   // windowed tiles (layer longer than the tile)
    int gn_npt = 0;          // > 0: a windowed GroupNorm'd layer, finished by gn_pass_kernel<gn_npt> after the conv
    SplitPlan split{1, 0, 0};
    uint64_t xswz = 0;
    bool halo8 = false;      // launched as conv_halo8_f32<BM, SK, fused> (choose_halo8), not as the conv-GEMM kernel above
    uint64_t xswz8 = 0;      //   its slot shifts (find_xswz_pairs)
    bool halo8w = false;     //   ... in its register-weight form conv_halo8w_f32, with
    size_t lds8w_bytes = 0;  //   that form's dynamic LDS (X rows only: halo8w_lds_floats)
};

// The general staging path (RAGGED kernels): a K chunk may straddle the concat's seam or the end of the channels, or
// a source's rows are not whole float4s.
inline bool ragged_operands(const ConvOp& op, int kc) {
    const int cin = op.cin0 + op.cin1;
    return (op.cin0 & 3) != 0 || (op.cin1 & 3) != 0 || op.cin0 % kc != 0 || cin % kc != 0;
}
// Does the residual conv ride in `op`'s launch, given its tile and grid-level split?  (Needs the whole K in one
// block and the sixth tap's weight rows in LDS.)  The one statement of the rule: a 1x1 residual conv is launched
// on its own exactly where its carrier's LaunchGeom::fused is false (plan_forward).
inline bool fused_at(const HostModel& m, const ConvOp& op, const LaunchGeom& g) {
    if (!op.ride || !m.fuse_residual || g.cfg < 0) return false;
    const TileCfg& t = kTiles[g.cfg];
    if (t.KC < 16 || g.split.kslices != 1) return false;
    // Tile 5's ride with whole K chunks (conv_gemm_f32<32, 64, 2, 16, k, 1, RAGGED = false, RES>) computes wrong values
    // ("Forward kernel census"; tests/test_hip_forward_paths.py): the 1x1 conv is launched on its own there.
    if (g.cfg == 5 && !ragged_operands(op, g.kc)) return false;
    return dad::conv_lds_floats(t.BM, t.BN, g.kc, op.taps, op.Lin, op.Lout, t.SK, false, op.taps + 1) *
               sizeof(float) <= dad::kLdsBytes;
}
// What a launch of `op` at this batch is made of: tile, K chunk, grid-level split-K, whether the residual conv
// rides.  Scratch is sized from these alone, so a size does not depend on whether plan_launch accepts the launch.
inline void choose_launch(const HostModel& m, const ConvOp& op, int batch, LaunchGeom& g) {
    g = LaunchGeom();
    g.cfg = choose_tile(m, op, batch);
    if (g.cfg < 0) return;
    g.kc = tile_kc(g.cfg, op.taps, op.x3, op.bdir);
    g.split = plan_split(m, op, g.cfg, batch);
    g.fused = fused_at(m, op, g);
}

// Which conv-GEMM instantiations exist.  This is the one statement of it: the registry of dad_lib.hip
// (kernel_table) is generated by walking this predicate's domain at compile time and instantiates a kernel where it
// is true and nowhere else, and the planner — and the sanitizer harness, which has no device code — refuses a launch
// it is false for.  dad_debug_kernel_table_consistent() checks that the generated table covers the domain and
// holds nothing else.  The domain: tile 0..kNumTiles-1, taps 1..kRegMaxTaps, stride 1..2, kRegFlags flags (kFamilies,
// at the end of this file, lists it with the other families' and holds the count).
constexpr int kRegMaxTaps = 7;
constexpr int kRegFlags = 6;      // x3, bdir, ragged, res, padded, windowed: bits 0..5 of a flag word
constexpr bool kernel_registered(int cfg, int taps, int stride, bool x3, bool bdir, bool ragged, bool res, bool padded = false,
                                 bool windowed = false) {
    if (cfg < 0 || cfg >= kNumTiles) return false;
    if (windowed) {
        if (!kWinTiles[cfg] || !padded || x3 || bdir || res) return false;
        const bool odd = taps == 3 || taps == 5 || taps == 7 || taps == 1;
        if (ragged) return stride == 1 && odd;
        return (stride == 1 && (odd || taps == 2)) || (stride == 2 && (taps == 3 || (taps == 5 && kTiles[cfg].KC >= 16)));
    }
    if (padded && (!kPaddedTiles[cfg] || x3 || res)) return false;
    const bool kc16 = kTiles[cfg].KC >= 16;
    const bool k357 = taps == 3 || taps == 5 || taps == 7;
    if (ragged && !(stride == 1 && (k357 || taps == 1) && !bdir)) return false;
    if (bdir) return !kc16 && !res && !ragged && stride == 1 && k357;
    if (res) return kc16 && !x3 && stride == 1 && k357;
    if (x3) return kc16 && ((taps == 5 && stride == 1) || (taps == 3 && stride == 2) || (taps == 2 && stride == 1) ||
                            (taps == 1 && stride == 1));
    if (stride == 2) return taps == 3 || (taps == 5 && kc16);
    return stride == 1 && (taps == 1 || taps == 2 || k357);
}
// the same with the six flags as one word (how the registry and its check walk the domain)
constexpr bool kernel_registered_f(int cfg, int taps, int stride, int f) {
    return kernel_registered(cfg, taps, stride, f & 1, f & 2, f & 4, f & 8, f & 16, f & 32);
}

inline int plan_launch(const HostModel& m, const ConvOp& op, int batch, LaunchGeom& g) {
    choose_launch(m, op, batch, g);
    if ((long)batch * op.Lout * op.M >= (1L << 31) ||
        (long)batch * op.Lin * (op.cin0 + op.cin1) >= (1L << 31))
        return fail(DAD_E_INVALID, "batch %d too large: a layer's activation tensor exceeds 2^31 elements", batch);
    if (g.cfg < 0)
        return fail(DAD_E_INVALID, "no tile configuration for %s (M=%d, C/8=%d, L=%d)",
                    op.name.c_str(), op.M, op.cout / 8, op.Lout);
    const TileCfg& t = kTiles[g.cfg];
    const int cin = op.cin0 + op.cin1;
    g.ragged = ragged_operands(op, g.kc);
    if (g.ragged && !(op.stride == 1 && (op.taps & 1) == 1))
        return fail(DAD_E_INVALID, "channel count %d+%d needs the general staging path, which exists "
                    "for stride-1 k-tap and 1x1 convs only", op.cin0, op.cin1);
    if (op.bdir && g.ragged)
        return fail(DAD_E_INVALID, "the direct-B kernel needs whole 32-channel chunks (%d+%d)", op.cin0, op.cin1);
    if (op.bdir && !(t.KC == 8 && op.kind == CONV_K5 && op.stride == 1))
        return fail(DAD_E_INVALID, "no direct-B kernel for tile %d taps=%d stride=%d", g.cfg, op.taps, op.stride);
    if (op.x3 && !op.bdir && t.KC < 16)
        return fail(DAD_E_INVALID, "no split-f16 kernel for tile %d taps=%d stride=%d", g.cfg, op.taps, op.stride);
    if (g.fused && (op.x3 || op.bdir || op.kind != CONV_K5 || op.stride != 1))
        return fail(DAD_E_INVALID, "no fused-residual kernel for %s on tile %d", op.name.c_str(), g.cfg);
    if (op.cin_pad % g.kc != 0 && !g.ragged)
        return fail(DAD_E_INVALID, "%s: padded channel count %d is not a multiple of the K chunk %d",
                    op.name.c_str(), op.cin_pad, g.kc);
    g.windowed = op.Lout > t.BN;
    g.padded = op.net_padded || g.windowed;
    if (!kernel_registered(g.cfg, op.taps, op.stride, op.x3, op.bdir, g.ragged, g.fused, g.padded, g.windowed))
        return fail(DAD_E_INVALID, "no kernel for %s (tile %d taps=%d stride=%d x3=%d bdir=%d ragged=%d res=%d padded=%d windowed=%d)",
                    op.name.c_str(), g.cfg, op.taps, op.stride, (int)op.x3, (int)op.bdir, (int)g.ragged, (int)g.fused, (int)g.padded,
                    (int)g.windowed);
    if (g.windowed && !op.norm.empty() && (long)(op.cout / 8) * op.Lout > kGnPassMaxPair)
        return fail(DAD_E_INVALID, "%s: GroupNorm pair of %ld elements (the pass holds %d)", op.name.c_str(),
                    (long)(op.cout / 8) * op.Lout, kGnPassMaxPair);
    if (g.windowed && !op.norm.empty()) {
        const long elems = (long)(op.cout / 8) * op.Lout, per = dad::GNP_THREADS * 4L;     // per: elements per float4 of every thread
        if (op.kind != CONV_K5 || (op.cout / 8) % 4 != 0)
            return fail(DAD_E_INVALID, "%s: no GroupNorm pass for %ld-element pairs", op.name.c_str(), elems);
        for (g.gn_npt = 1; elems > g.gn_npt * per; g.gn_npt *= 2) {}
    }
    g.threads = 64 * (t.BM / 32) * (t.BN / 32) * t.SK;
    g.lds_bytes = dad::conv_lds_floats(t.BM, t.BN, g.kc, op.taps, op.Lin, op.Lout, t.SK, op.bdir,
                                       op.taps + (g.fused ? 1 : 0)) * sizeof(float);
    if (g.lds_bytes > dad::kLdsBytes)
        return fail(DAD_E_INVALID, "%s: tile %d needs %zu bytes of LDS", op.name.c_str(), g.cfg, g.lds_bytes);
    const long ntn = tiles_n(op, t.BN, batch);
    if (ntn > 65535) return fail(DAD_E_INVALID, "batch too large for one launch (%ld N tiles)", ntn);
    g.ntiles_n = (int)ntn;
    g.mtiles = op.M / t.BM;
    if (g.split.kslices > 1 && (long)g.mtiles * g.ntiles_n > kMaxSplitTiles)
        return fail(DAD_E_INVALID, "%s: %ld tiles exceed the split-K ticket table", op.name.c_str(),
                    (long)g.mtiles * g.ntiles_n);
    // XCD-aware tile order when every XCD gets the same whole rectangle of tiles: choose the
    // gm x gn arrangement of the 8 XCDs that minimises  gn * (weight bytes) + gm * (activation bytes)
    const int MT = g.mtiles, NTn = g.ntiles_n;
    g.gx = (unsigned)g.split.kslices; g.gy = (unsigned)MT; g.gz = (unsigned)NTn;
    g.xcd_gn = 0;
    if (m.xcd_order && g.split.kslices == 1 && (MT & (MT - 1)) == 0 && (long)MT * NTn <= 65535 &&
        ((long)MT * NTn) % 8 == 0) {
        const double wbytes = (double)op.M * op.taps * cin;
        const double xbytes = (double)batch * op.Lin * cin;
        double best = -1;
        for (int gm = 1; gm <= 8; gm *= 2) {
            const int gn = 8 / gm;
            if (MT % gm != 0 || NTn % gn != 0) continue;
            const double cost = gn * wbytes + gm * xbytes;
            if (best < 0 || cost < best) {
                best = cost;
                g.xcd_gn = gn; g.xcd_mts = ilog2(MT / gm); g.xcd_ntn = NTn / gn;
            }
        }
        if (g.xcd_gn > 0) { g.gy = (unsigned)(MT * NTn); g.gz = 1; }
    }
    g.xswz = m.xswz_enabled ? find_xswz(m, op.Lout, op.stride, op.taps / 2, (g.kc + 4) / 4, t.BN) : 0;
    return DAD_OK;
}

// conv_halo8.hpp: which launches of a forward evaluation take the halo-skipping kernel instead of the conv-GEMM
// kernel plan_launch chose.  It exists for the 5-tap stride-1 fp32 convs of 8-position layers on tiles 0 and 1,
// with whole aligned K chunks and no grid split-K, and is taken only in the full-chip regime (kSplitMaxTiles output
// tiles or more) of the heuristic: a forced tile (dad_debug_set_tile, split-K switched off included) pins the
// conv-GEMM kernels and their summation order.  Not for the training forward (plan_forward applies it to m.plan
// only).  The ride is decided by fused_at as before.
// Which conv_halo8_f32 instantiations exist, by (tile cfg, the launch carries a riding 1x1 conv): the block tiles of
// kTiles[0 / 1], each with and without the ride.
constexpr bool halo8_kernel_exists(int cfg, bool /*ride*/) { return cfg == 0 || cfg == 1; }
// ... on this tile at all, with the ride or without
constexpr bool halo8_kernel_exists(int cfg) { return halo8_kernel_exists(cfg, false) || halo8_kernel_exists(cfg, true); }
inline bool halo8_layer(const ConvOp& op) {
    return op.kind == CONV_K5 && op.taps == 5 && op.stride == 1 && op.Lin == 8 && op.Lout == 8 && !op.x3 && !op.bdir &&
           !op.net_padded && !op.padded() && op.pre < 0 && op.stats < 0;
}
// The register-weight form conv_halo8w_f32 exists wherever conv_halo8_f32 does; which of the two a launch takes by
// default is the measurement of DESIGN.md section 3 ("Weights straight into MFMA registers"), per (tile, ride).
constexpr bool halo8w_faster(int cfg, bool /*ride*/) { return cfg == 0 || cfg == 1; }
inline void choose_halo8(const HostModel& m, const ConvOp& op, LaunchGeom& g) {
    g.halo8 = false; g.xswz8 = 0; g.halo8w = false; g.lds8w_bytes = 0;
    if (!m.halo8_enabled || m.force_tile >= 0 || !m.split_enabled || g.cfg < 0 || !halo8_layer(op)) return;
    if (!halo8_kernel_exists(g.cfg, g.fused) || g.kc != 32 || g.ragged || g.padded || g.windowed || g.split.kslices != 1) return;
    if ((long)g.mtiles * g.ntiles_n < kSplitMaxTiles) return;
    g.halo8 = true;
    g.xswz8 = m.xswz_enabled ? find_xswz_pairs(m, op.Lout, op.taps / 2, (g.kc + 4) / 4) : 0;
    g.halo8w = m.halo8_wreg < 0 ? halo8w_faster(g.cfg, g.fused) : m.halo8_wreg != 0;
    if (g.halo8w) g.lds8w_bytes = dad::halo8w_lds_floats(kTiles[g.cfg].BM, kTiles[g.cfg].SK) * sizeof(float);
}

// ------------------------------------------------------------------ small-batch (CC) plan
// conv_cc.hpp: convs only produce partial sums, consumers finish them.  Decided per batch on the
// host: which launches exist, their K slices, where their partial slabs live, and for every input
// whether it is read finished (external trajectory / already materialised) or in pieces.
constexpr int kCcMaxSlabs = 16;          // slabs a consumer adds (8 per round trip)
constexpr int kCcMaxSlice = 64;          // channels per K slice of conv_cc: weight tile + input slice stay well
                                         // inside LDS and 6 float4 of weights per thread
constexpr int kCcwMaxSlabs = 8;          // conv_ccw (wide layers): slabs per input, one round trip
using dad::kCcwMaxPairs;
constexpr int kCcwMaxPair = 8192;        // elements of one pair (up to 2048 stay in registers between the passes)
struct CcInput {
    int kind = 0;            // 0 none, 1 external trajectory, 2 finished tensor in a plan buffer, 3 in pieces
    int buf = -1;            // kind 2 / 3: the tensor's activation buffer (kind 3: where it is materialised)
    int producer = -1;       // kind 3: conv whose partial slabs these are
};
struct CcOp {
    bool launched = false;   // false: the op does not exist in this form (riding 1x1 conv)
    bool wide = false;       // conv_ccw.hpp: weights streamed through registers, K slices of up to 1024 channels
    int slice_ch = 0, kslices = 0, ntiles = 0;
    int tile_rows = 32;      // GEMM rows per tile: 16 for layers of at most 16 positions (16x16x4 MFMAs)
    bool big = false;        // an input arrives in more than CC_MAX_SLABS slabs (conv_cc's second round trip)
    bool ride_in = false;    // an input's residual is a 1x1 conv still in pieces (conv_ccw's RIDE form)
    long oslab = 0, orslab = -1;       // float offsets into the CC slab region
    int out_rows = 0, out_cols = 0;
    size_t lds_bytes = 0;
    CcInput in0, in1;
    // how this conv's OUTPUT is finished by whoever consumes it
    int res_kind = 0;        // 0 none, 1 external trajectory, 2 finished tensor (buffer res_buf),
                             // 3 ride of conv res_ride, 4 the stand-alone 1x1 conv res_ride, still in pieces
    int res_buf = -1, res_ride = -1;
};
struct CcPlan {
    bool ok = false;
    std::vector<CcOp> ops;
    long slab_floats = 0;
    int final_producer = -1;
    std::string why;         // when !ok: which rule refused the plan (diagnostic)
};
inline CcPlan& refuse(CcPlan& P, const char* why) { P.why = why; return P; }
// Which small-batch conv kernels exist: conv_cc, and (`wide`) conv_ccw (`rows` per tile; `ride`: the launch carries a
// riding 1x1 conv; conv_ccw has every form of `ride_in`).  The registry of dad_lib.hip is generated from it (kFamilies).
constexpr bool cc_kernel_exists(int taps, int stride, bool ride, bool wide, bool big, int rows, bool windowed) {
    if ((rows != 16 && rows != 32) || (ride && !(taps == 5 && stride == 1))) return false;
    const bool shape_ok = (taps == 5 && stride == 1) || (taps == 3 && stride == 2) || (taps == 2 && stride == 1);
    if (wide) return !big && !windowed && (shape_ok || (taps == 1 && stride == 1));   // a wide conv takes at most CC_MAX_SLABS slabs
    if (windowed) return taps == 5 && stride == 1 && !big && rows == 32;
    return shape_ok;
}

inline CcPlan cc_plan(const HostModel& m, int batch) {
    CcPlan P;
    const dad_cfg& c = m.cfg;
    const std::vector<ConvOp>& convs = m.plan.convs;
    if (m.precision != DAD_PREC_FP32 || !m.cc_enabled || c.horizon > 128 || c.kernel_size != 5 ||
        (long)batch * c.horizon > m.cc_max_rows)
        return refuse(P, "disabled, split-f16 arithmetic, horizon > 128, kernel_size != 5 or more than cc_max_rows rows");
    // horizons beyond 32 (windowed tiles): measured on the PointMaze net at horizon 64 — 258 / 260 / 272 us per denoise
    // step at batch 1 / 2 / 4 against 282 / 293 / 314 on the batch kernels; at batch 8 the batch kernels win
    if (c.horizon > 32 && (long)batch * c.horizon > 256)
        return refuse(P, "horizon > 32 and more than 256 rows");
    for (const ConvOp& op : convs)
        if (op.gn_real > 0) return refuse(P, "zero-padded GroupNorm groups (dad_model_set_group_channels): batch kernels only");
    if (m.real_horizon > 0 && m.real_horizon != c.horizon) return refuse(P, "zero-padded horizon (dad_model_set_horizon): batch kernels only");
    for (const ConvOp& op : convs)      // weight images in 16-channel granules only
        if ((op.kc != 16 && !op.bdir) || op.cat0 >= 0 || op.x3 || (!op.rname.empty() && !op.ride)) return refuse(P, "a weight image not in 16-channel granules, or an identity residual over a concat");
    P.ops.resize(convs.size());
    std::vector<int> owner(m.plan.bufs.size(), -1);     // buffer -> conv whose output it holds
    std::vector<char> materialised(convs.size(), 0);
    long off = 0;
    for (size_t i = 0; i < convs.size(); ++i) {
        const ConvOp& op = convs[i];
        CcOp& o = P.ops[i];
        if (op.rider_of >= 0) { owner[op.dst] = -2 - op.rider_of; continue; }   // lives in its carrier's launch
        o.launched = true;
        // inputs
        auto input = [&](int buf, CcInput& in) -> bool {
            if (buf == -1) { in.kind = 0; return true; }
            if (buf == -2) { in.kind = 1; return true; }
            const int q = owner[buf];
            if (q < 0) return false;                     // unknown producer (should not happen)
            in.buf = buf;
            if (materialised[q]) { in.kind = 2; return true; }
            in.kind = 3; in.producer = q; materialised[q] = 1;
            return true;
        };
        if (!input(op.src0, o.in0) || !input(op.src1, o.in1)) return refuse(P, "input with no known producer");
        // layers of more than 32 positions (horizon 64 / 128): windowed tiles — 32 rows of one sample per tile,
        // stride-1 5-tap convs of conv_cc only (the pair statistics still span the sample: <= 1024 elements)
        const bool windowed = op.Lout > 32;
        if (op.M % 32 != 0 || (!windowed && 32 % op.Lout != 0) || (windowed && (op.Lout % 32 != 0 || op.kind != CONV_K5)))
            return refuse(P, "output columns not a multiple of 32, a length that does not divide 32, or a long layer that is not a stride-1 conv");
        // K slices: whole GroupNorm groups of the tensor being finished
        const int cin = op.cin0 + op.cin1;
        int need = 32, max_slabs_in = 0;
        long max_pair = 0;
        for (const CcInput* in : {&o.in0, &o.in1})
            if (in->kind == 3) {
                const ConvOp& q = convs[in->producer];
                const CcOp& qo = P.ops[in->producer];
                max_slabs_in = std::max(max_slabs_in, qo.kslices);
                if (qo.res_kind >= 3) max_slabs_in = std::max(max_slabs_in, P.ops[qo.res_ride].kslices);
                o.ride_in = o.ride_in || qo.res_kind >= 3;
                if (!q.norm.empty()) {
                    need = std::max(need, q.cout / 8);
                    max_pair = std::max(max_pair, (long)(q.cout / 8) * op.Lin);
                    if (need % (q.cout / 8) != 0) return refuse(P, "inputs whose GroupNorm widths do not nest");          // slices must hold whole groups
                }
            }
        int slice = need;
        while ((cin + slice - 1) / slice > 8 && slice < kCcMaxSlice) slice *= 2;     // 8 slabs: one round trip
        while ((cin + slice - 1) / slice > kCcMaxSlabs) slice *= 2;
        // conv_cc keeps the whole weight slice in LDS and normalises a pair in one wave's registers;
        // anything wider goes to conv_ccw (weights streamed global -> registers)
        o.wide = slice > kCcMaxSlice || max_pair > 1024 || op.bdir || op.kind == CONV_1X1;   // (conv_cc has no 1x1 form)
        if (o.wide && (windowed || op.Lin > 32)) return refuse(P, "a wide layer (conv_ccw) of more than 32 positions");
        if (windowed && max_slabs_in > 8) return refuse(P, "a windowed layer fed more than 8 slabs");
        if (!o.wide) {
            if (slice % 32 != 0) return refuse(P, "K slice not a multiple of 32 channels");
            // 16-row tiles (16x16x4 MFMAs, half the padded rows) as long as the layer still fits one wave
            // of blocks; beyond that the extra N tiles only re-stream the weights
            o.tile_rows = 32;
            if (op.Lout <= 16) {
                const int ks = (cin + slice - 1) / slice;
                const long blocks16 = (long)((batch + 16 / op.Lout - 1) / (16 / op.Lout)) * (op.M / 32) * ks;
                if (blocks16 <= 256) o.tile_rows = 16;
            }
        } else {
            if (op.src0 == -2 || (op.cin0 & 3) || (op.cin1 & 3) || max_slabs_in > kCcwMaxSlabs ||
                max_pair > kCcwMaxPair)
                return refuse(P, "wide layer: ragged channels, more than 8 slabs to add, or a GroupNorm pair above 8192 elements");
            // tile rows: 16 when that needs no more N tiles than 32 would (batch 1 / 2 on short levels),
            // or when a 32-row tile of the narrowest admissible slice does not fit LDS
            auto try_rows = [&](int rows) -> int {
                auto fits = [&](int sl) {
                    return dad::ccw_lds_floats(sl, op.taps, op.Lin, op.Lout, rows) * sizeof(float) <= dad::kLdsBytes;
                };
                const int spt_r = rows / op.Lout;
                const long nt = (batch + spt_r - 1) / spt_r;
                int sl = need;
                while (sl % 32 != 0) sl += need;
                while ((cin + sl - 1) / sl > kCcwMaxSlabs) sl *= 2;
                // fewer, fatter slices while the chip stays covered: every slab is re-read by all the M
                // tiles of its consumer
                while ((long)((cin + 2 * sl - 1) / (2 * sl)) * (op.M / 32) * nt >= m.ccw_min_blocks && 2 * sl <= cin && fits(2 * sl) &&
                       (op.cin1 == 0 || op.cin0 % (2 * sl) == 0))
                    sl *= 2;
                return fits(sl) ? sl : 0;
            };
            o.tile_rows = 32;
            if (op.Lout <= 16 && (batch + 16 / op.Lout - 1) / (16 / op.Lout) == (batch + 32 / op.Lout - 1) / (32 / op.Lout))
                o.tile_rows = 16;
            slice = try_rows(o.tile_rows);
            if (o.tile_rows == 32 && op.Lout <= 16 && m.ccw_prefer16) {
                // LDS-short 32-row tiles end up with twice the K slices (twice the slabs for the consumer
                // to add); two 16-row tiles re-read the weights from L2 instead
                const int s16 = try_rows(16);
                if (slice == 0 || s16 >= 2 * slice) { o.tile_rows = 16; slice = s16; }
            }
            if (slice == 0) return refuse(P, "wide layer: no K slice of at most 8 slabs fits LDS");
            const int spt_w = o.tile_rows / op.Lout;
            int min_cpg = slice;
            for (const CcInput* in : {&o.in0, &o.in1})
                if (in->kind == 3 && !convs[in->producer].norm.empty())
                    min_cpg = std::min(min_cpg, convs[in->producer].cout / 8);
            if ((long)spt_w * (slice / min_cpg) > kCcwMaxPairs) return refuse(P, "wide layer: more than 64 (sample, group) pairs per block");
        }
        if (op.cin1 > 0 && op.cin0 % slice != 0) return refuse(P, "a K slice would straddle the concat");     // a slice may not straddle the concat
        o.slice_ch = slice;
        o.kslices = (cin + slice - 1) / slice;
        if ((long)o.kslices * slice > op.cin_pad) return refuse(P, "weight image too short for whole K slices");    // weight image too short for whole slices
        // a (sample, group) pair of the output is normalised by its consumer: conv_cc / final_cc take at
        // most 1024 elements per pair, conv_ccw 8192 (checked again where the consumer is planned)
        if (!op.norm.empty() && (long)(op.cout / 8) * op.Lout > kCcwMaxPair) return refuse(P, "GroupNorm pair above 8192 elements");
        const int spt = windowed ? 1 : o.tile_rows / op.Lout;
        o.ntiles = windowed ? batch * (op.Lout / 32) : (batch + spt - 1) / spt;
        o.out_rows = op.kind == CONV_UP ? batch * 2 * op.Lout : batch * op.Lout;
        o.out_cols = op.kind == CONV_UP ? op.M / 2 : op.M;
        o.oslab = off;
        off += (long)o.kslices * o.out_rows * o.out_cols;
        if (op.ride) { o.orslab = off; off += (long)o.kslices * o.out_rows * o.out_cols; }
        o.lds_bytes = (o.wide ? dad::ccw_lds_floats(slice, op.taps, op.Lin, op.Lout, o.tile_rows)
                              : dad::cc_lds_floats(slice, op.taps, op.wtaps(), op.Lin, op.Lout, o.tile_rows)) * sizeof(float);
        if (o.lds_bytes > dad::kLdsBytes) return refuse(P, "a launch does not fit LDS");
        o.big = max_slabs_in > dad::CC_MAX_SLABS;
        if (!cc_kernel_exists(op.taps, op.stride, op.ride, o.wide, o.big, o.tile_rows, windowed)) return refuse(P, "a launch no small-batch kernel exists for");
        // how the output gets finished
        if (op.res == -2) o.res_kind = 1;
        else if (op.res >= 0) {
            const int q = owner[op.res];
            if (q <= -2) { o.res_kind = 3; o.res_ride = -2 - q; }
            else if (q >= 0 && materialised[q]) { o.res_kind = 2; o.res_buf = op.res; }
            else if (q >= 0 && convs[q].kind == CONV_1X1 && convs[q].norm.empty() && P.ops[q].launched) {
                o.res_kind = 4; o.res_ride = q;          // the block's own 1x1 residual conv, still in pieces
            } else return refuse(P, "residual tensor neither finished nor a 1x1 conv in pieces");                             // residual not finished yet: not a plan we know
        }
        owner[op.dst] = (int)i;
    }
    P.final_producer = owner[m.plan.final_act];
    if (P.final_producer < 0 || materialised[P.final_producer]) return refuse(P, "final conv input already finished");
    // the streamed-weight form re-reads the weights once per N tile: measured against the batch-256
    // kernels it pays up to 4 plans of 32 positions (HalfCheetah 410 / 627 us per step at batch 1 / 4
    // against 597 / 653; 973 against 683 at batch 6)
    for (const CcOp& o : P.ops)
        if (o.launched && o.wide && (long)batch * c.horizon > m.ccw_max_rows) return refuse(P, "wide layers and more than ccw_max_rows rows");
    {   // final_cc_kernel normalises a pair in one wave's registers
        const ConvOp& f = convs[P.final_producer];
        if ((long)(f.cout / 8) * f.Lout > 1024) return refuse(P, "final conv: GroupNorm pair above 1024 elements");
        // (final_cc_kernel finishes its input with cc_build_input<false>: one round of CC_MAX_SLABS = 8 slabs)
        if (P.ops[P.final_producer].kslices > 8) return refuse(P, "final conv: more than 8 partial slabs");
    }
    P.slab_floats = off;
    P.ok = true;
    return P;
}

// ------------------------------------------------------------------ one forward evaluation at a batch
// Planning goes on after a refusal (the sizes are reported for such a batch too); the first one is what is returned.
struct FirstRefusal {
    int rc = DAD_OK;
    std::string why;
    void note(int r) { if (r != DAD_OK && rc == DAD_OK) { rc = r; why = g_err; } }
    int done() const { return rc == DAD_OK ? DAD_OK : fail(rc, "%s", why.c_str()); }
};
// rows per sample of the external tensors (x, noise, guide, means): the horizon before zero-padding
inline int traj_horizon(const HostModel& m) { return m.real_horizon > 0 ? m.real_horizon : m.cfg.horizon; }

struct FwdLaunch {
    int conv;                // index into the plan's convs
    bool ok;                 // plan_launch accepted it
    LaunchGeom g;
};
// Everything one denoiser evaluation launches at a batch, decided before its first launch: every entry point builds
// it once per call (plan_forward) and replays it; the size queries, the plan report and the sanitizer harness read it.
struct FwdPlan {
    bool train = false;      // the launches of m.tplan (dad_unet_forward_train), else of m.plan
    int batch = 0;
    CcPlan cc;               // cc.ok: the evaluation takes the small-batch kernels, `launches` stays empty
    std::vector<FwdLaunch> launches;     // else the conv-GEMM launches in order; a 1x1 residual conv that rides at
                                         // this batch (its carrier's g.fused) is absent
    unsigned final_gx = 1, final_gy = 1; // final_cc_kernel / final_posterior_kernel
    size_t final_lds = 0;
    size_t bytes = 0;        // activations + the scratch behind them: split-K slabs or the small-batch slabs,
                             // whichever is larger (a small batch with per-row timesteps runs the batch kernels)
};
// `small_ok`: the call may take the small-batch kernels (one shared timestep, not training).  `f` is filled even
// when a launch is refused, and the refusal returned: dad_workspace_bytes / dad_train_workspace_bytes report the
// sizes, the launching entry points refuse before their first launch.
inline int plan_forward(const HostModel& m, bool train, int batch, bool small_ok, FwdPlan& f) {
    const Plan& plan = train ? m.tplan : m.plan;
    const dad_cfg& c = m.cfg;
    FirstRefusal first;
    f = FwdPlan();
    f.train = train; f.batch = batch;
    long scratch = 0;
    if (!train) {
        CcPlan cc = cc_plan(m, batch);
        if (cc.ok) scratch = cc.slab_floats;
        if (cc.ok && small_ok) f.cc = std::move(cc);
    }
    std::vector<char> carries(plan.convs.size(), 0);
    for (size_t i = 0; i < plan.convs.size(); ++i) {
        const ConvOp& op = plan.convs[i];
        FwdLaunch l{(int)i, true, LaunchGeom()};
        const bool listed = !f.cc.ok && !(op.rider_of >= 0 && carries[op.rider_of]);
        if (listed) { const int rc = plan_launch(m, op, batch, l.g); l.ok = rc == DAD_OK; first.note(rc); }
        else choose_launch(m, op, batch, l.g);         // (its split-K slab still counts: sizes are one rule for all calls)
        if (listed && l.ok && !train) choose_halo8(m, op, l.g);
        carries[i] = l.g.fused;
        scratch = std::max(scratch, l.g.split.slab_floats);
        if (listed) f.launches.push_back(l);
    }
    f.bytes = ((size_t)plan.floats_per_sample * (size_t)batch + (size_t)scratch) * sizeof(float);
    if (f.cc.ok) {
        // one block per (sample, group of output columns): enough columns per block to occupy its
        // 512 threads once, as long as the grid stays within one wave of blocks
        const int want = (c.horizon * c.transition_dim + dad::CC_THREADS - 1) / dad::CC_THREADS;
        f.final_gx = (unsigned)batch;
        f.final_gy = (unsigned)std::max(1, std::min({want, c.transition_dim, 256 / std::max(batch, 1)}));
        f.final_lds = dad::final_cc_lds_floats(c.transition_dim, c.dim, c.horizon) * sizeof(float);
    } else {
        // columns of the transition are spread over gridDim.y when the row tiles alone leave CUs idle
        // (a block stages only the weight rows of its own columns), and further until a block fits LDS
        const long row_tiles = ((long)batch * traj_horizon(m) + dad::FINAL_COLS - 1) / dad::FINAL_COLS;
        const long col_groups = (c.transition_dim + 256 / dad::FINAL_COLS - 1) / (256 / dad::FINAL_COLS);
        long gy = std::max(1L, std::min(col_groups, 512 / row_tiles));
        while (gy < col_groups && dad::final_lds_floats(c.transition_dim, c.dim, (int)gy) * sizeof(float) > dad::kLdsBytes) ++gy;
        f.final_gx = (unsigned)row_tiles; f.final_gy = (unsigned)gy;
        f.final_lds = dad::final_lds_floats(c.transition_dim, c.dim, (int)gy) * sizeof(float);
    }
    if (f.final_lds > dad::kLdsBytes)
        first.note(fail(DAD_E_INVALID, "final 1x1 conv does not fit LDS (td=%d, dim=%d)", c.transition_dim, c.dim));
    return first.done();
}
inline size_t workspace_bytes(const HostModel& m, int batch) {
    FwdPlan f;
    plan_forward(m, false, batch, true, f);
    return f.bytes;
}

// ------------------------------------------------------------------ the seam between two steps of dad_sample_loop
// conv_seam.hpp: final_conv[1] + the posterior update of step t and the first conv of the evaluation at t - 1 (with
// its riding 1x1 residual conv) as one launch, in place of final_posterior_kernel and the evaluation's first listed
// launch.  Decided once per dad_sample_loop call, from the call's FwdPlan and arguments; this is the one statement of
// the rule (dad_debug_seam_plan reports it).  Everything it refuses runs the launches of the FwdPlan as they are.
// The first condition that fails, in this order, is the reason:
enum SeamWhy {
    SEAM_TAKEN = 0,
    SEAM_OPTION,          // dad_debug_set_option("step_seam", 0)
    SEAM_SMALL_BATCH,     // the evaluation takes the small-batch kernels (conv_cc.hpp), not the batch kernels
    SEAM_PRECISION,       // split-f16 arithmetic
    SEAM_FORCED_TILE,     // dad_debug_set_tile pins the conv-GEMM kernels (split-K switched off included)
    SEAM_PROJECTION,      // the projection sits between the posterior and the next evaluation
    SEAM_PADDED,          // zero-padded horizon or GroupNorm groups
    SEAM_HORIZON,         // a 32-row tile holds whole samples: 8, 16 or 32 positions
    SEAM_TRANSITION_DIM,  // one 16-channel granule
    SEAM_DIM,             // no instantiation for this dim on either tile (seam_kernel_exists)
    SEAM_FIRST_CONV,      // the first launch is not the 5-tap transition_dim -> dim Conv1dBlock of one K chunk
    SEAM_NO_RIDE,         // the 1x1 residual conv does not ride in it (fused_at)
    SEAM_TILE,            // no instantiation for its tile (neither 0 nor 1, or seam_kernel_exists): the launch keeps the tile's
                          //   summation and reduction order, and has them for these two (tile 2, from 512 N tiles on, owns
                          //   eight float4 per thread)
    SEAM_LDS,
    SEAM_BUFFERS,         // final_act against the buffers the conv and the ride write (seam_buffers_ok)
    SEAM_WHYS
};
inline const char* seam_reason(int why) {
    static const char* const names[SEAM_WHYS] = {"taken", "option off", "small-batch kernels", "split-f16 arithmetic", "forced tile",
                                                 "projection", "zero-padded net", "horizon", "transition_dim", "dim", "first conv",
                                                 "no riding residual conv", "tile", "LDS", "buffers"};
    return why >= 0 && why < SEAM_WHYS ? names[why] : "?";
}
struct SeamPlan {
    int why = SEAM_OPTION;
    bool tile0 = false;      // the first conv's tile is 0 (else 1): conv_seam_f32<dim, tile0>
    int cfg = -1;
    int units = 0;           // 8-channel units with real channels
    unsigned grid = 0;
    int threads = 0;
    size_t lds_bytes = 0;
    uint64_t xswz = 0;       // slot shifts of its X stage
    // what the report adds (dad_debug_seam_plan); the launch reads none of them
    int dim = 0;             // conv_seam_f32<dim, tile0>
    int spt = 0;             // samples of one 32-row tile
    int last = 0;            // samples in the last tile, 1 .. spt
    int buffers = -1;        // seam_buffer_relation
    bool taken() const { return why == SEAM_TAKEN; }
};
// Which conv_seam_f32 instantiations exist, by (dim, the first conv's tile is 0, else 1): tile 1 holds 64 output
// channels, so it starts at dim 64.
constexpr int kSeamDims[] = {32, 64, 128};
constexpr bool seam_kernel_exists(int dim, bool tile0) {
    for (int d : kSeamDims)
        if (d == dim) return tile0 || dim >= 64;
    return false;
}
// The launch reads final_act and writes the first conv's dst and rdst.  The activation allocator reuses buffer ids:
// final_conv[0] is handed the first free level-0 buffer, which on every net so far is the first conv's own.  Allowed:
// three buffers whose floats do not overlap — or final_act being the very buffer (same id, so same offset) the conv
// or the ride writes: both sides are then [B * H][dim] row-major, and a workgroup reads its 32 rows in full before it
// writes those 32 rows and no others (conv_seam.hpp).  Any other overlap is refused.
inline bool seam_buffers_ok(const Plan& plan, const ConvOp& op) {
    const int n = (int)plan.bufs.size();
    const int fa = plan.final_act;
    if (fa < 0 || fa >= n || op.dst < 0 || op.dst >= n || op.rdst < 0 || op.rdst >= n || op.dst == op.rdst) return false;
    const long rows = (long)op.Lout * op.M;         // floats per sample the launch reads / writes of each
    auto apart = [&](int a, int b) {
        const long a0 = plan.bufs[a].offset, b0 = plan.bufs[b].offset;
        return a0 + rows <= b0 || b0 + rows <= a0;
    };
    for (int id : {fa, op.dst, op.rdst})
        if (plan.bufs[id].per_sample < rows) return false;
    if (!apart(op.dst, op.rdst)) return false;
    for (int id : {op.dst, op.rdst})
        if (id != fa && !apart(fa, id)) return false;
    return true;
}
// Which of the relations seam_buffers_ok allows holds (DAD_SEAM_BUF_* of include/dad.h), -1 where it allows none.
inline int seam_buffer_relation(const Plan& plan, const ConvOp& op) {
    if (!seam_buffers_ok(plan, op)) return -1;
    return plan.final_act == op.dst ? DAD_SEAM_BUF_DST : plan.final_act == op.rdst ? DAD_SEAM_BUF_RDST : DAD_SEAM_BUF_APART;
}
inline SeamPlan plan_seam(const HostModel& m, const FwdPlan& f, bool projection) {
    SeamPlan s;
    const dad_cfg& c = m.cfg;
    const int H = c.horizon, td = c.transition_dim, dim = c.dim;
    auto no = [&](int why) { s.why = why; return s; };
    if (!m.step_seam) return no(SEAM_OPTION);
    if (f.train || f.cc.ok || f.launches.empty()) return no(SEAM_SMALL_BATCH);
    if (m.precision != DAD_PREC_FP32) return no(SEAM_PRECISION);
    if (m.force_tile >= 0 || !m.split_enabled) return no(SEAM_FORCED_TILE);
    if (projection) return no(SEAM_PROJECTION);
    const FwdLaunch& l = f.launches[0];
    const ConvOp& op = m.plan.convs[l.conv];
    if (traj_horizon(m) != H || op.net_padded || op.padded()) return no(SEAM_PADDED);
    if (H != 8 && H != 16 && H != 32) return no(SEAM_HORIZON);
    if (td > 16) return no(SEAM_TRANSITION_DIM);
    if (!seam_kernel_exists(dim, true) && !seam_kernel_exists(dim, false)) return no(SEAM_DIM);
    const LaunchGeom& g = l.g;
    if (l.conv != 0 || !l.ok || op.kind != CONV_K5 || op.taps != 5 || op.stride != 1 || op.src0 != -2 || op.src1 >= 0 || op.cin0 != td ||
        op.cin1 != 0 || op.cout != dim || op.M != dim || op.Lin != H || op.Lout != H || op.norm.empty() || op.res != -1 || op.cat0 >= 0 ||
        op.x3 || op.bdir || op.kc != 16 || op.cin_pad < 16 || g.halo8 || g.padded || g.windowed || g.split.kslices != 1)
        return no(SEAM_FIRST_CONV);
    if (!g.fused || op.rdst < 0) return no(SEAM_NO_RIDE);
    if ((g.cfg != 0 && g.cfg != 1) || g.kc != 32 || !seam_kernel_exists(dim, g.cfg == 0)) return no(SEAM_TILE);
    s.lds_bytes = dad::seam_lds_floats(td, dim, H) * sizeof(float);
    if (s.lds_bytes > dad::kLdsBytes) return no(SEAM_LDS);
    if (!seam_buffers_ok(m.plan, op)) return no(SEAM_BUFFERS);
    s.cfg = g.cfg;
    s.tile0 = g.cfg == 0;
    s.units = td > 8 ? 2 : 1;
    s.grid = (unsigned)(((long)f.batch * H + 31) / 32);
    s.threads = dad::seam_threads(dim);
    s.xswz = m.xswz_enabled ? find_xswz(m, H, 1, 2, dad::SEAM_KP / 4, 32) : 0;
    s.dim = dim;
    s.spt = 32 / H;
    s.last = f.batch - ((int)s.grid - 1) * s.spt;
    s.buffers = seam_buffer_relation(m.plan, op);
    s.why = SEAM_TAKEN;
    return s;
}

// ------------------------------------------------------------------ projection: which kernel, on which grid
// One call of dad_project / dad_projection_violation (run_project launches from this; dad_debug_project_plan reports
// it).  D = (H+1) n + H m, x_bytes: the batch of trajectories, scratch_bytes: dad_project_args.scratch (0 without one).
struct ProjectPlan {
    int form = DAD_PP_ROW1;  // DAD_PP_ROW1 project_kernel<1,16>, DAD_PP_ROW4 project_kernel<4,16>, DAD_PP_GEMM project_gemm_kernel
    int rows_per_block = 1;
    unsigned gx = 1, gy = 1;
    size_t lds_bytes = 0;
    bool refused = false;    // one trajectory's partial sums exceed LDS and the GEMM form is not to be had
};
inline ProjectPlan plan_project(int D, int batch, size_t x_bytes, size_t scratch_bytes, bool violation) {
    ProjectPlan q;
    // batches of 32+ trajectories with scratch for the projected copy: v @ P as an MFMA GEMM (P read once
    // per 32 trajectories, not once per trajectory)
    // (at PointMaze size, D = 196, the per-trajectory kernel is the faster one: 10 us against 16.6 us for
    // 256 plans — 56 GEMM blocks leave most of the chip idle; the GEMM takes over from D = 512)
    const size_t row_lds = dad::project_row_lds_bytes(D);             // a row + its 16 partial sets
    const bool gemm_pays = D >= 512 || row_lds > dad::kLdsBytes;
    if (!violation && gemm_pays && batch >= 32 && scratch_bytes > 0 && scratch_bytes >= x_bytes) {
        q.form = DAD_PP_GEMM;
        q.rows_per_block = 32;
        q.gx = (unsigned)((batch + 31) / 32); q.gy = (unsigned)((D + 31) / 32);
        q.lds_bytes = dad::project_gemm_lds_floats() * sizeof(float);
        return q;
    }
    // rows per block: one while the batch fits one wave of blocks (every CU streams P once),
    // four beyond that (P is then re-used by four rows per pass) if four rows fit LDS
    const int rb = (batch > 512 && 4 * row_lds <= dad::kLdsBytes) ? 4 : 1;
    q.form = rb == 4 ? DAD_PP_ROW4 : DAD_PP_ROW1;
    q.rows_per_block = rb;
    q.gx = (unsigned)((batch + rb - 1) / rb);
    q.lds_bytes = rb * row_lds;
    q.refused = q.lds_bytes > dad::kLdsBytes;
    return q;
}

// ------------------------------------------------------------------ violation gradient: which form, on which grids
// One dad_projection_violation_fwd / _bwd pair (run_violation_fwd / _bwd launch from this; dad_debug_violation_grad_plan
// reports it).  D as above, row_elems = H (od + m): one trajectory of x, form: -1 the rule below, 0 row, 1 gemm.
struct ViolationGradPass {
    int rows_per_block = 1;
    unsigned gx = 1, gy = 1;
    size_t lds_bytes = 0;
    unsigned tail_gx = 0;    // forward: violation_sum_kernel, backward: violation_scatter_kernel (gemm form only)
};
struct ViolationGradPlan {
    int form = DAD_VG_ROW;
    ViolationGradPass fwd, bwd;
    int col_blocks = 0;                          // gemm: 32-column blocks of P = partial sums per trajectory
    size_t r_off = 0, part_off = 0, g_off = 0;   // where r (B, D), the partial sums and g (B, D) start, in floats
    size_t workspace_bytes = 0;
    bool refused = false;    // a forced row form whose forward LDS (a row + its 16 partial sets) exceeds a CU's
};
// The projection's own crossover: the GEMM form from D = 512 at batches of 32+, and wherever a row does not fit LDS.
// (Measured for this pair, DESIGN.md §3 "Violation gradient": the row form is faster at D = 196 (19.5 us against 31.0 us
// of kernel time at B = 256) and still 6 us ahead at D = 514; the GEMM form is 3.3 x faster at D = 2183.  The crossover
// between 514 and 2183 was not measured, so the constant is not moved.)
constexpr int kViolationGemmMinD = 512;
constexpr int kViolationGemmMinBatch = 32;
inline ViolationGradPlan plan_violation_grad(int D, int batch, long row_elems, int form) {
    ViolationGradPlan q;
    const size_t row_lds = dad::project_row_lds_bytes(D);
    const bool row_fits = row_lds <= dad::kLdsBytes;
    const bool gemm = form < 0 ? (!row_fits || (D >= kViolationGemmMinD && batch >= kViolationGemmMinBatch)) : form == 1;
    const auto round64 = [](size_t floats) { return (floats + 63) / 64 * 64; };       // sections start 256 bytes aligned
    const size_t bd = (size_t)batch * (size_t)D;
    if (!gemm) {
        // forward: project_kernel's violation branch exactly as dad_projection_violation plans it (same bits), with
        // the residual kept; backward: one block per trajectory
        const ProjectPlan f = plan_project(D, batch, 0, 0, true);
        q.form = DAD_VG_ROW;
        q.fwd.rows_per_block = f.rows_per_block; q.fwd.gx = f.gx; q.fwd.gy = f.gy; q.fwd.lds_bytes = f.lds_bytes;
        q.bwd.rows_per_block = 1; q.bwd.gx = (unsigned)batch; q.bwd.gy = 1;
        q.bwd.lds_bytes = dad::vg_row_bwd_lds_bytes(D);
        q.refused = f.refused || q.bwd.lds_bytes > dad::kLdsBytes;
        q.workspace_bytes = round64(bd) * sizeof(float);
        return q;
    }
    q.form = DAD_VG_GEMM;
    q.col_blocks = (D + 31) / 32;
    q.fwd.rows_per_block = q.bwd.rows_per_block = 32;
    q.fwd.gx = q.bwd.gx = (unsigned)((batch + 31) / 32);
    q.fwd.gy = q.bwd.gy = (unsigned)q.col_blocks;
    q.fwd.lds_bytes = dad::project_gemm_lds_floats() * sizeof(float);
    q.bwd.lds_bytes = dad::vg_gemm_bwd_lds_floats() * sizeof(float);
    q.fwd.tail_gx = (unsigned)((batch + dad::VG_TAIL_THREADS - 1) / dad::VG_TAIL_THREADS);
    q.bwd.tail_gx = (unsigned)(((size_t)batch * (size_t)row_elems + dad::VG_TAIL_THREADS - 1) / dad::VG_TAIL_THREADS);
    q.part_off = round64(bd);
    q.g_off = q.part_off + round64((size_t)batch * (size_t)q.col_blocks);
    q.workspace_bytes = (q.g_off + round64(bd)) * sizeof(float);
    return q;
}

// ------------------------------------------------------------------ library guide: which nets, on which grid
// One launch of guide_mlp_kernel (guide_mlp.hpp): dad_guide_grad and every guide launch of dad_guided_loop launch
// from this, dad_debug_guide_plan reports it.  The net is in_dim -> widths[0] -> ... -> widths[n_layers - 1]; the
// limits are the GM_* constants of conv_shapes.hpp and a CU's LDS, in the order of DAD_GD_REFUSALS.
struct GuidePlan {
    int n_layers = 0;
    int padded[dad::GM_MAX_LAYERS] = {0, 0, 0, 0};    // padded[0]: in_dim; padded[i + 1]: hidden widths[i]
    int rows_per_block = dad::GM_ROWS;
    int threads = dad::GM_THREADS;
    unsigned gx = 0;
    size_t lds_bytes = 0;
    int refused = DAD_GD_OK;
};
inline GuidePlan plan_guide(int in_dim, const int* widths, int n_layers, int activation, int batch, int horizon, int td) {
    GuidePlan q;
    q.n_layers = n_layers;
    q.gx = (unsigned)(((long)batch * horizon + dad::GM_ROWS - 1) / dad::GM_ROWS);
    q.padded[0] = in_dim > 0 ? dad::guide_pad(in_dim) : 0;
    const auto no = [&](int why) { q.refused = why; return q; };
    if (n_layers < dad::GM_MIN_LAYERS || n_layers > dad::GM_MAX_LAYERS || widths == nullptr) return no(DAD_GD_BAD_LAYERS);
    for (int i = 0; i < n_layers; ++i)
        if (widths[i] < 1 || widths[i] > dad::GM_MAX_WIDTH) return no(DAD_GD_BAD_WIDTH);
    for (int i = 0; i + 1 < n_layers; ++i) q.padded[i + 1] = dad::guide_pad(widths[i]);
    if (activation != DAD_GD_TANH && activation != DAD_GD_RELU && activation != DAD_GD_MISH) return no(DAD_GD_BAD_ACT);
    if (in_dim < 1 || in_dim > td) return no(DAD_GD_BAD_IN_DIM);
    if (widths[n_layers - 1] != 1) return no(DAD_GD_BAD_LAST);
    q.lds_bytes = dad::guide_lds_floats(in_dim, widths, n_layers, activation == DAD_GD_MISH) * sizeof(float);
    if (q.lds_bytes > dad::kLdsBytes) return no(DAD_GD_BAD_LDS);
    return q;
}
// The checks on the shape every entry point of the guide makes before it plans
inline int guide_shape_checked(int batch, int horizon, int td) {
    if (batch <= 0 || horizon <= 0 || td <= 0)
        return fail(DAD_E_INVALID, "guide: batch=%d, horizon=%d, transition_dim=%d must be positive", batch, horizon, td);
    if ((long)batch * horizon * td > (long)INT32_MAX)
        return fail(DAD_E_INVALID, "guide: batch=%d x horizon=%d x transition_dim=%d exceeds 2^31 elements", batch, horizon, td);
    return DAD_OK;
}
inline const char* guide_refusal(int why) {
    switch (why) {
        case DAD_GD_BAD_LAYERS: return "the net must have 2 to 4 Linear layers";
        case DAD_GD_BAD_WIDTH: return "every width must lie in 1 .. 512";
        case DAD_GD_BAD_ACT: return "unknown activation (DAD_GD_TANH, DAD_GD_RELU, DAD_GD_MISH)";
        case DAD_GD_BAD_IN_DIM: return "in_dim must lie in 1 .. transition_dim";
        case DAD_GD_BAD_LAST: return "the last layer must have one output";
        case DAD_GD_BAD_LDS: return "the kept tensors of 32 rows exceed one CU's LDS";
    }
    return "";
}

// ------------------------------------------------------------------ backward pass: per-batch geometry
// Which conv_wgrad instantiations exist, by (taps, block tile, windowed: layers longer than a chunk stages): these tap
// counts, each on tile 0 = 64 x 64 (two K-groups), 1 = 64 x 32 (four), 2 = 32 x 32 (eight) and 3 = 32 x 32 with the
// general staging path (operands that are not whole aligned float4 rows), plain and windowed.
constexpr int kWgradTaps[] = {1, 3, 4, 5, 7};
constexpr int kWgradTiles = 4;
constexpr bool wgrad_kernel_exists(int taps, int tile, bool /*windowed*/) {
    for (int t : kWgradTaps)
        if (t == taps) return tile >= 0 && tile < kWgradTiles;
    return false;
}
struct WgradGeom { int spc, ksplit, sps, tile, tm, tn; unsigned gx, gy; size_t lds; };
// Layers longer than a chunk stages (more than 128 rows of G or Z per sample: horizons 256 / 512) run the windowed
// kernel over windows of kWgradWindow rows of G (and the matching rows of Z) as if they were samples.
constexpr int kWgradWindow = 64;
struct WgradShape { int B, Lg, Lz, wshift; };
inline WgradShape wgrad_shape(int B, int Lg, int Lz) {
    if (Lg <= 128 && Lz <= 128) return {B, Lg, Lz, 0};
    const int nw = Lg / kWgradWindow;
    return {B * nw, kWgradWindow, Lz / nw, ilog2(nw)};
}
// Block tile: the largest of 64 x 64 / 64 x 32 / 32 x 32 that still gives the layer 32 tiles (the smaller tiles
// split K inside the block instead of over the grid: fewer partial slabs to write and add); the batch is then split
// over blockIdx.z until `target` blocks exist (one block = 8 waves = two per SIMD).
inline WgradGeom wgrad_geom(int M, int Ctot, int B, int Lg, int Lz, int taps, int pad, int target, bool ragged) {
    WgradGeom g{};
    g.spc = std::max(1, dad::WG_ROWS / Lg);
    while (g.spc > 1 && g.spc * dad::wgrad_segz(Lz, taps, pad) > dad::WG_MAX_ZROWS) g.spc /= 2;
    static const int tms[3] = {2, 2, 1}, tns[3] = {2, 1, 1};
    long tiles = 0;
    for (g.tile = ragged ? 2 : 0; g.tile < 3; ++g.tile) {
        g.tm = tms[g.tile]; g.tn = tns[g.tile];
        g.gx = (unsigned)((M + 32 * g.tm - 1) / (32 * g.tm));
        g.gy = (unsigned)((Ctot + 32 * g.tn - 1) / (32 * g.tn));
        tiles = (long)g.gx * g.gy;
        const int kgroups = 8 / (g.tm * g.tn);
        if ((tiles >= 32 && (g.spc * Lg) % (4 * kgroups) == 0) || g.tile == 2) break;
    }
    const int chunks = (B + g.spc - 1) / g.spc;
    int want = (int)std::max(1L, target / tiles);
    want = std::min(want, chunks);
    g.sps = (chunks + want - 1) / want * g.spc;                // samples per split: whole chunks
    g.ksplit = (B + g.sps - 1) / g.sps;
    g.lds = dad::wgrad_lds_floats(g.spc, Lg, Lz, taps, pad, g.tm, g.tn) * sizeof(float);
    if (ragged) g.tile = 3;
    return g;
}

// Scratch of dad_unet_backward, in floats: gradient mirror of the training plan | per-sample partial sums
// | wgrad split slabs | padded d x | staging of a down-sampling conv's data gradient | split-K slabs;
// and the geometry of every weight-gradient and every data-gradient step of m.bsteps, each in order.
struct TrainScratch {
    long mirror = 0, part = 0, wslab = 0, dxpad = 0, tmp = 0, bslab = 0, total = 0;
    struct Wgrad { WgradShape sh; WgradGeom g; };
    struct Dgrad { bool ok; LaunchGeom g; };       // ok: plan_launch accepted it
    std::vector<Wgrad> wgrads;
    std::vector<Dgrad> dgrads;
};
inline const ConvOp& bwd_op(const HostModel& m, const BwdStep& s) { return s.conv < 0 ? m.bfinal : m.bconvs[s.conv].op[s.sub]; }
// Everything of the backward pass that depends on the batch, with every check of its launches.  `t` is filled even
// when a check fails: dad_train_workspace_bytes reports the sizes, dad_unet_backward refuses before its first launch.
inline int train_scratch(const HostModel& m, int B, TrainScratch& t) {
    const int H = m.cfg.horizon, td = m.cfg.transition_dim;
    FirstRefusal first;
    t = TrainScratch();
    t.mirror = m.tplan.floats_per_sample * (long)B;
    for (const ConvOp& f : m.tplan.convs) t.part += (f.norm.empty() ? 1L : 3L) * B * round_up(f.cout, 4);
    t.part += (long)B * round_up(td, 4);
    for (const BwdStep& s : m.bsteps) {
        if (s.kind == BK_WGRAD) {
            const WgradShape sh = wgrad_shape(B, s.Lg, s.Lz);             // windows of long layers run as samples
            const bool ragged = ((s.M | s.C0 | s.C1) & 3) != 0;          // rows that are not whole aligned float4s
            const WgradGeom g = wgrad_geom(s.M, s.C0 + s.C1, sh.B, sh.Lg, sh.Lz, s.taps, s.pad, m.wgrad_blocks, ragged);
            const long numel = (long)s.M * (s.C0 + s.C1) * s.taps;
            const int kgroups = 8 / (g.tm * g.tn);
            if (g.lds > dad::kLdsBytes || g.spc * sh.Lg > dad::WG_MAX_GROWS ||
                g.spc * dad::wgrad_segz(sh.Lz, s.taps, s.pad) > dad::WG_MAX_ZROWS || (g.spc * sh.Lg) % (4 * kgroups) != 0)
                first.note(fail(DAD_E_INVALID, "wgrad: a chunk of %d samples x %d rows does not fit the kernel's staging", g.spc, sh.Lz));
            if (!wgrad_kernel_exists(s.taps, g.tile, sh.wshift > 0))
                first.note(fail(DAD_E_INVALID, "wgrad: %d taps", s.taps));
            if (g.ksplit > 1 && numel % 4 != 0)
                first.note(fail(DAD_E_INVALID, "wgrad: %ld gradient elements (not a multiple of 4)", numel));
            if (g.ksplit > 1) t.wslab = std::max(t.wslab, (long)g.ksplit * numel);
            t.wgrads.push_back({sh, g});
        } else if (s.kind == BK_DGRAD) {
            const ConvOp& op = bwd_op(m, s);
            TrainScratch::Dgrad d{};
            const int rc = plan_launch(m, op, B, d.g);
            d.ok = rc == DAD_OK;
            first.note(rc);
            t.bslab = std::max(t.bslab, d.g.split.slab_floats);
            t.dgrads.push_back(d);
            if (op.kind == CONV_UP) t.tmp = std::max(t.tmp, (long)B * s.n);
        }
    }
    t.dxpad = (long)B * H * round_up(td, 32);
    if (m.real_horizon > 0 && m.real_horizon != H) t.dxpad += 2L * B * H * round_up(td, 4);      // zero-padded copies of x and d out
    auto al = [](long v) { return (v + 63) / 64 * 64; };
    t.mirror = al(t.mirror); t.part = al(t.part); t.wslab = al(t.wslab); t.dxpad = al(t.dxpad);
    t.tmp = al(t.tmp); t.bslab = al(t.bslab);
    t.total = t.mirror + t.part + t.wslab + t.dxpad + t.tmp + t.bslab;
    if (m.bpart * B > t.part)
        first.note(fail(DAD_E_WORKSPACE, "backward: partial sums overran their region (%ld > %ld floats)", m.bpart * B, t.part));
    return first.done();
}

// ---- the fused training objective (dad_train_objective_forward / dad_train_objective_backward)
// What it keeps beyond the training forward's activations and the backward pass's scratch: offsets in floats from
// the start of the new part of `saved` / `scratch`, which begins at the next multiple of 256 bytes behind the
// existing part; every region starts at a multiple of 64 floats.
struct ObjectiveLayout {
    // saved: written by the forward, read by the backward
    long xt = 0, out = 0, t_rows = 0, row_index = 0, h1 = 0, temb = 0, act = 0, rows = 0, partial = 0, saved_floats = 0;
    // scratch: the backward pass's own
    long d_out = 0, d_rows = 0, dact_slab = 0, dtemb = 0, dh1 = 0, scratch_floats = 0;
    int loss_blocks = 1;     // blocks of the loss's partial sums
    int kslices = 1;         // K slices of d act = d rows . W (K = temb_width), added in slice order
    int kslice = 0;          //   columns per slice (a multiple of 128: 32 per wave)
    size_t saved_base = 0, scratch_base = 0;      // bytes of the existing parts (rounded up to 256)
    size_t saved_bytes = 0, scratch_bytes = 0;    // totals: what dad_train_objective_workspace_bytes reports
};
constexpr int kObjectiveMaxLossBlocks = 1024;
// One launch of the time chain (csrc/train_objective.hpp): out[M][N] = sum over K, `kslices` slices of `kslice` k values
// over blockIdx.z.  mode: DAD_OP_TG_* of include/dad.h (the TimeGemm of time_gemm_kernel; DAD_OP_TG_DTEMB: the slab
// sum time_dtemb_kernel, M x N elements over K = kslices slabs).
struct TimeLaunch {
    int mode, M, N, K, kslice, kslices;
    unsigned gx() const { return mode == DAD_OP_TG_DTEMB ? (unsigned)(((long)M * N + 255) / 256) : (unsigned)((M + 31) / 32); }
    unsigned gy() const { return mode == DAD_OP_TG_DTEMB ? 1u : (unsigned)((N + 31) / 32); }
    unsigned gz() const { return mode == DAD_OP_TG_DTEMB ? 1u : (unsigned)kslices; }
};
constexpr int kObjectiveForwardLaunches = 3, kObjectiveTimeLaunches = 9;
// Everything one objective call plans on the host, planned once: the layout, the training forward it replays,
// (`backward`) the geometry of the backward pass, which dad_unet_backward's body takes over instead of planning again,
// and the time chain's launches in launch order (`time`: 3 forward, 6 backward; the entry points only replay them).
// Without `backward` the scratch half of the layout stays empty (the forward does not touch `scratch`).
struct ObjectivePlan { ObjectiveLayout o; FwdPlan fwd; TrainScratch ts; std::vector<TimeLaunch> time; };
inline int objective_plan(const HostModel& m, int B, bool backward, ObjectivePlan& p) {
    ObjectiveLayout& o = p.o;
    FwdPlan& f = p.fwd;
    TrainScratch& ts = p.ts;
    o = ObjectiveLayout();
    FirstRefusal first;
    first.note(plan_forward(m, true, B, false, f));
    ts = TrainScratch();
    if (backward) first.note(train_scratch(m, B, ts));
    const long tdm = m.cfg.time_dim, W = std::max(1, m.tplan.temb_width);
    const long n = (long)B * traj_horizon(m) * m.cfg.transition_dim;
    auto al = [](long v) { return (v + 63) / 64 * 64; };
    o.loss_blocks = (int)std::max(1L, std::min((long)kObjectiveMaxLossBlocks, (n + 1023) / 1024));
    const long tiles = (long)((B + 31) / 32) * ((tdm + 31) / 32);
    const long want = std::max(1L, std::min(256 / tiles, (W + 127) / 128));
    o.kslice = (int)(((W + want - 1) / want + 127) / 128 * 128);
    o.kslices = (int)((W + o.kslice - 1) / o.kslice);
    long at = 0;
    auto take = [&](long floats) { const long q = at; at += al(floats); return q; };
    o.xt = take(n); o.out = take(n); o.t_rows = take(B); o.row_index = take(B);
    o.h1 = take(B * 4 * tdm); o.temb = take(B * tdm); o.act = take(B * tdm); o.rows = take(B * W);
    o.partial = take(o.loss_blocks);
    o.saved_floats = at;
    at = 0;
    o.d_out = take(n); o.d_rows = take(B * W); o.dact_slab = take((long)o.kslices * B * tdm);
    o.dtemb = take(B * tdm); o.dh1 = take(B * 4 * tdm);
    o.scratch_floats = at;
    o.saved_base = (f.bytes + 255) / 256 * 256;
    o.scratch_base = ((size_t)ts.total * sizeof(float) + 255) / 256 * 256;
    o.saved_bytes = o.saved_base + (size_t)o.saved_floats * sizeof(float);
    o.scratch_bytes = o.scratch_base + (size_t)o.scratch_floats * sizeof(float);
    {
        const int t1 = m.cfg.time_dim, t4 = 4 * t1, E = m.cfg.dim, Wt = m.tplan.temb_width;
        p.time = {
            {DAD_OP_TG_FWD_H1, B, t4, E, E, 1},                     // h1 = emb W1^T + b1
            {DAD_OP_TG_FWD_TEMB, B, t1, t4, t4, 1},                 // temb = mish(h1) W3^T + b3, act = mish(temb)
            {DAD_OP_TG_FWD_ROWS, B, Wt, t1, t1, 1},                 // rows = act Wk^T + bk, all blocks
            {DAD_OP_TG_BWD_DWK, Wt, t1, B, B, 1},                   // d Wk = d rows^T act, d bk
            {DAD_OP_TG_BWD_DACT, B, t1, Wt, o.kslice, o.kslices},   // d act = d rows W, K slices in slabs
            {DAD_OP_TG_DTEMB, B, t1, o.kslices, o.kslices, 1},      // d temb = (sum of the slabs) mish'(temb)
            {DAD_OP_TG_BWD_DW3, t1, t4, B, B, 1},                   // d W3 = d temb^T mish(h1), d b3
            {DAD_OP_TG_BWD_DH1, B, t4, t1, t1, 1},                  // d h1 = (d temb W3) mish'(h1)
            {DAD_OP_TG_BWD_DW1, t4, E, B, B, 1},                    // d W1 = d h1^T emb, d b1
        };
    }
    if ((int)time_block_list(m).size() > 4 * DAD_MAX_LEVELS)
        first.note(fail(DAD_E_INVALID, "objective: %zu residual blocks", time_block_list(m).size()));
    return first.done();
}
inline int objective_layout(const HostModel& m, int B, ObjectiveLayout& o) {
    ObjectivePlan p;
    const int rc = objective_plan(m, B, true, p);
    o = p.o;
    return rc;
}

// ---- the dynamics-aware objective (dad_train_dynamics_objective_forward / _backward): the fused objective above plus
// the violation of the predicted plan x0_hat, sharing t, the noise, x_t and `out`
// What it keeps beyond the fused objective's regions: offsets in floats from the start of its own part of `saved` /
// `scratch`, which begins at the next multiple of 256 bytes behind the objective's; regions start at multiples of 64
// floats.  One launch of its own kernels (csrc/train_objective.hpp) per DynLaunch, forward ones first.
struct DynLaunch { int kind; unsigned gx, gy; int threads; size_t lds_bytes; int rows_per_block; };
struct DynamicsObjectivePlan {
    ObjectivePlan obj;
    ViolationGradPlan vg;        // the form and the grids: plan_violation_grad's, for x0_hat's shape
    int D = 0, horizon = 0;      // (H + 1) n + H m for the trajectories' real horizon H
    // saved: the residual r (B, D) | gemm form: sums of r^2 per (trajectory, column block) | row form: violation (B)
    long r = 0, part = 0, violation = 0, saved_floats = 0;
    long g = 0, scratch_floats = 0;      // scratch: gemm form: g (B, D)
    size_t saved_base = 0, scratch_base = 0;      // bytes of the fused objective's parts (rounded up to 256)
    size_t saved_bytes = 0, scratch_bytes = 0;    // totals: what dad_train_dynamics_objective_workspace_bytes reports
    int fwd_launches = 0;
    std::vector<DynLaunch> launches;
};
// `form`: -1 planned, 0 row, 1 gemm (as dad_projection_violation_fwd).  The shape is checked first; a forced row form
// beyond a CU's LDS is planned (vg.refused) and refused by the entry points, as the violation pair does.
inline int dynamics_objective_plan(const HostModel& m, int B, int state_dim, int observation_dim, int action_dim, int form,
                                   bool backward, DynamicsObjectivePlan& p) {
    p = DynamicsObjectivePlan();
    if (B <= 0) return fail(DAD_E_INVALID, "dynamics objective: batch must be positive (got %d)", B);
    if (state_dim <= 0 || action_dim <= 0 || state_dim > observation_dim)
        return fail(DAD_E_INVALID, "dynamics objective: state_dim=%d must lie in 1 .. observation_dim=%d, action_dim=%d be positive",
                    state_dim, observation_dim, action_dim);
    if (observation_dim + action_dim != m.cfg.transition_dim)
        return fail(DAD_E_INVALID, "dynamics objective: observation_dim=%d + action_dim=%d is not the model's transition_dim=%d",
                    observation_dim, action_dim, m.cfg.transition_dim);
    if (form < -1 || form > 1) return fail(DAD_E_INVALID, "dynamics objective: form=%d is none of -1 (planned), 0 (row), 1 (gemm)", form);
    const int H = traj_horizon(m), td = m.cfg.transition_dim;
    const long D = (long)(H + 1) * state_dim + (long)H * action_dim;
    if (D > INT32_MAX / 64) return fail(DAD_E_INVALID, "projection dimension D=%ld too large", D);
    p.D = (int)D; p.horizon = H;
    const int rc = objective_plan(m, B, backward, p.obj);
    p.vg = plan_violation_grad(p.D, B, (long)H * td, form);
    auto al = [](long v) { return (v + 63) / 64 * 64; };
    long at = 0;
    auto take = [&](long floats) { const long q = at; at += al(floats); return q; };
    const bool gemm = p.vg.form == DAD_VG_GEMM;
    p.r = take((long)B * D);
    if (gemm) p.part = take((long)B * p.vg.col_blocks); else p.violation = take(B);
    p.saved_floats = at;
    at = 0;
    if (gemm) p.g = take((long)B * D);
    p.scratch_floats = at;
    p.saved_base = (p.obj.o.saved_bytes + 255) / 256 * 256;
    p.scratch_base = (p.obj.o.scratch_bytes + 255) / 256 * 256;
    p.saved_bytes = p.saved_base + (size_t)p.saved_floats * sizeof(float);
    p.scratch_bytes = p.scratch_base + (size_t)p.scratch_floats * sizeof(float);
    const ViolationGradPass &f = p.vg.fwd, &b = p.vg.bwd;
    if (gemm) {
        p.launches = {{DAD_DO_K_FWD_GEMM, f.gx, f.gy, dad::PG_THREADS, f.lds_bytes, 32},
                      {DAD_DO_K_FWD_PARTS, 1, 1, 256, 0, 0},
                      {DAD_DO_K_BWD_GEMM, b.gx, b.gy, dad::PG_THREADS, b.lds_bytes, 32},
                      {DAD_DO_K_BWD_SCATTER, b.tail_gx, 1, dad::VG_TAIL_THREADS, 0, 0}};
    } else {
        p.launches = {{DAD_DO_K_FWD_ROW, f.gx, f.gy, 64 * dad::PROJ_KP, f.lds_bytes, f.rows_per_block},
                      {DAD_DO_K_FWD_PARTS, 1, 1, 256, 0, 0},
                      {DAD_DO_K_BWD_ROW, b.gx, b.gy, 64 * dad::VG_ROW_WAVES, b.lds_bytes, 1}};
    }
    p.fwd_launches = 2;
    return rc;
}

// What a BK_GN step hands gn_mish_bwd_kernel / gn_mish_bwd_wave_kernel besides its pointers: read from the forward conv
// the step belongs to.  dad_unet_backward fills GnBwdParams from it, backward_steps_encode writes it down.
struct GnBwdShape { int C, L, cpg, lreal, cpg_real; bool dtemb; };
inline GnBwdShape gn_bwd_shape(const ConvOp& f) { return {f.cout, f.Lout, f.cout / 8, f.lreal, f.gn_real, f.temb_off >= 0}; }
// The col_sums_many_kernel launches that end a pass: bsums in order, at most dad::COLS_MAX per launch.
inline int col_sums_launches(const HostModel& m) { return (int)((m.bsums.size() + dad::COLS_MAX - 1) / dad::COLS_MAX); }

// The small-batch kernels of one launch, whichever of the two families it takes: conv_cc has no `ride_in` form (a
// consumer of ride slabs runs the same instantiation), conv_ccw (`wide`) neither `big` nor `windowed`.
constexpr bool small_kernel_exists(int taps, int stride, bool ride, bool wide, bool big, bool ride_in, int rows, bool windowed) {
    if (wide) return !big && cc_kernel_exists(taps, stride, ride, true, false, rows, windowed);
    return !ride_in && cc_kernel_exists(taps, stride, ride, false, big, rows, windowed);
}

// ------------------------------------------------------------------ the kernel families
// Every family of instantiated kernels the library looks up at launch time: its key, the finite domain the key ranges
// over, and — family_kernel_exists — the predicate above that says where in the domain a kernel exists.  The registry of
// dad_lib.hip is generated from this table alone (one compile-time walk per family instantiates a kernel where the
// predicate holds and nowhere else), the planner asks the same predicates, and dad_debug_kernel_table_consistent()
// walks every domain against the generated table.  A new family is one predicate and one line here, plus the line of
// dad_lib.hip (kernel_of) that names its template.
enum KernelFamily {
    FAM_GEMM = DAD_FAMILY_GEMM,       // conv_gemm_f32   (cfg, taps, stride, flags)                    kernel_registered_f
    FAM_CC = DAD_FAMILY_CC,           // conv_cc         (taps, stride, ride, big, rows, windowed)     cc_kernel_exists
    FAM_CCW = DAD_FAMILY_CCW,         // conv_ccw        (taps, stride, ride, ride_in, rows)           cc_kernel_exists, wide
    FAM_HALO8 = DAD_FAMILY_HALO8,     // conv_halo8_f32  (cfg, ride)                                   halo8_kernel_exists
    FAM_SEAM = DAD_FAMILY_SEAM,       // conv_seam_f32   (dim, tile0)                                  seam_kernel_exists
    FAM_WGRAD = DAD_FAMILY_WGRAD,     // conv_wgrad      (taps, tile, windowed)                        wgrad_kernel_exists
    kNumFamilies = DAD_FAMILIES
};
constexpr int kMaxKeyInts = DAD_KERNEL_KEY_MAX;
// One axis of a domain: the `n` values lo, lo + 1, ..., or — with a list — values[0 .. n).
struct KeyAxis {
    int n, lo;
    const int* values;
    constexpr int at(int i) const { return values != nullptr ? values[i] : lo + i; }
    constexpr bool has(int v) const {
        if (values == nullptr) return v >= lo && v < lo + n;
        for (int i = 0; i < n; ++i)
            if (values[i] == v) return true;
        return false;
    }
};
struct FamilyDomain { const char* name; int count, axes; KeyAxis axis[kMaxKeyInts]; };
constexpr int kCcRows[] = {16, 32};
constexpr KeyAxis kTapsAxis = {kRegMaxTaps, 1, nullptr}, kStrideAxis = {2, 1, nullptr}, kBoolAxis = {2, 0, nullptr};
// 335 conv-GEMM kernels: 223 plain + 79 PADDED + 33 windowed (125 of them RAGGED).  Adding or dropping a kernel form
// changes a count here.
constexpr FamilyDomain kFamilies[kNumFamilies] = {
    {"conv_gemm_f32", 335, 4, {{kNumTiles, 0, nullptr}, kTapsAxis, kStrideAxis, {1 << kRegFlags, 0, nullptr}}},
    {"conv_cc", 18, 6, {kTapsAxis, kStrideAxis, kBoolAxis, kBoolAxis, {2, 0, kCcRows}, kBoolAxis}},
    {"conv_ccw", 20, 5, {kTapsAxis, kStrideAxis, kBoolAxis, kBoolAxis, {2, 0, kCcRows}}},
    {"conv_halo8_f32", 4, 2, {{kNumTiles, 0, nullptr}, kBoolAxis}},
    {"conv_seam_f32", 5, 2, {{(int)std::size(kSeamDims), 0, kSeamDims}, kBoolAxis}},
    {"conv_wgrad", 40, 3, {kTapsAxis, {kWgradTiles, 0, nullptr}, kBoolAxis}},
};
constexpr bool family_key_in_domain(int family, const int* k) {
    for (int a = 0; a < kFamilies[family].axes; ++a)
        if (!kFamilies[family].axis[a].has(k[a])) return false;
    return true;
}
// `k`: the family's key, kFamilies[family].axes ints
constexpr bool family_kernel_exists(int family, const int* k) {
    if (family < 0 || family >= kNumFamilies || !family_key_in_domain(family, k)) return false;
    switch (family) {
        case FAM_GEMM: return kernel_registered_f(k[0], k[1], k[2], k[3]);
        case FAM_CC: return cc_kernel_exists(k[0], k[1], k[2] != 0, false, k[3] != 0, k[4], k[5] != 0);
        case FAM_CCW: return cc_kernel_exists(k[0], k[1], k[2] != 0, true, false, k[4], false);     // every form of ride_in, k[3]
        case FAM_HALO8: return halo8_kernel_exists(k[0], k[1] != 0);
        case FAM_SEAM: return seam_kernel_exists(k[0], k[1] != 0);
        case FAM_WGRAD: return wgrad_kernel_exists(k[0], k[1], k[2] != 0);
    }
    return false;
}
inline bool family_kernel_exists(int family, std::initializer_list<int> k) {
    int key[kMaxKeyInts] = {};
    if (family < 0 || family >= kNumFamilies || (int)k.size() != kFamilies[family].axes) return false;
    std::copy(k.begin(), k.end(), key);
    return family_kernel_exists(family, key);
}
// The domain as a sequence: key number `index` of family_domain_size(family), the last axis running fastest.
constexpr int family_domain_size(int family) {
    int n = 1;
    for (int a = 0; a < kFamilies[family].axes; ++a) n *= kFamilies[family].axis[a].n;
    return n;
}
constexpr void family_key_at(int family, int index, int* k) {
    for (int a = kFamilies[family].axes - 1; a >= 0; --a) {
        const KeyAxis& ax = kFamilies[family].axis[a];
        k[a] = ax.at(index % ax.n);
        index /= ax.n;
    }
}
constexpr int count_family(int family) {
    int n = 0;
    for (int i = 0; i < family_domain_size(family); ++i) {
        int k[kMaxKeyInts] = {};
        family_key_at(family, i, k);
        n += family_kernel_exists(family, k);
    }
    return n;
}
static_assert(count_family(FAM_GEMM) == 335 && kFamilies[FAM_GEMM].count == 335, "the set of conv-GEMM kernels changed: kernel_registered");
static_assert(count_family(FAM_CC) == 18 && kFamilies[FAM_CC].count == 18, "the set of conv_cc kernels changed: cc_kernel_exists");
static_assert(count_family(FAM_CCW) == 20 && kFamilies[FAM_CCW].count == 20, "the set of conv_ccw kernels changed: cc_kernel_exists");
static_assert(count_family(FAM_HALO8) == 4 && kFamilies[FAM_HALO8].count == 4, "the set of conv_halo8_f32 kernels changed: halo8_kernel_exists");
static_assert(count_family(FAM_SEAM) == 5 && kFamilies[FAM_SEAM].count == 5, "the set of conv_seam_f32 kernels changed: seam_kernel_exists");
static_assert(count_family(FAM_WGRAD) == 40 && kFamilies[FAM_WGRAD].count == 40, "the set of conv_wgrad kernels changed: wgrad_kernel_exists");

// The flag word of kernel_registered_f for one launch: with (cfg, taps, stride) it names the conv_gemm_f32 instantiation.
inline int32_t launch_flags(const ConvOp& op, const LaunchGeom& g) {
    return (op.x3 ? 1 : 0) | (op.bdir ? 2 : 0) | (g.ragged ? 4 : 0) | (g.fused ? 8 : 0) | (g.padded ? 16 : 0) | (g.windowed ? 32 : 0);
}

// Bytes the parameter arena must hold: the parameter copies, the per-timestep tables, the zero row of the
// data-gradient launches, rng and split-K tickets.
inline size_t arena_bytes_needed(const HostModel& m, const std::vector<WeightEntry>& weights) {
    const dad_cfg& c = m.cfg;
    size_t floats = 0, allocs = 0;
    auto add = [&](size_t n) { floats += n + 64; ++allocs; };
    for (const WeightEntry& e : weights) add(e.size());
    const size_t T = c.n_timesteps;
    add(T * c.dim); add(T * 4 * c.time_dim); add(T * c.time_dim);
    add(T * std::max(1, m.plan.temb_width));
    if (m.training) add((size_t)std::max(m.max_bwd_m, 2 * m.max_cout) + 64);
    return floats * sizeof(float) + allocs * 256 + kMaxSplitTiles * sizeof(unsigned) + (1 << 16);
}

// SinusoidalPosEmb (temporal_unet.py:27-31) for every t in [0, T): fp32, in the reference's
// operation order (frequency = exp(j * -ln(1e4)/(half-1)) in fp32, argument = t * frequency).
inline std::vector<float> sinusoid_table(int T, int dim) {
    std::vector<float> emb((size_t)T * dim);
    const int half = dim / 2;
    const float scale = (float)(-(std::log(10000.0) / (half - 1)));
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < half; ++j) {
            const float f = std::exp((float)j * scale);
            const float arg = (float)t * f;
            emb[(size_t)t * dim + j] = std::sin(arg);
            emb[(size_t)t * dim + half + j] = std::cos(arg);
        }
    return emb;
}

// ------------------------------------------------------------------ optimiser step (dad_optim_step, csrc/optim_step.hpp)
// One step over a list of tensors is cut into chunks of kOptimChunk elements (the last chunk of a tensor is shorter;
// a chunk never spans two tensors, and starts at a multiple of 4 elements so that 16-byte accesses stay aligned).
// Chunks are numbered tensor by tensor; block b of the two kernels walks chunks [b * per_block, (b + 1) * per_block)
// in ascending order and finds the tensor of its first chunk by bisection over first[] (first[t] = first chunk of
// tensor t, first[n] = all chunks).  The square-sum pass writes one partial per block: partials == grid.
constexpr int kOptimChunk = 2048;        // elements: two float4 per thread of a 256-thread block
constexpr int kOptimMaxGrid = 2048;      // blocks of a memory-bound pass; beyond it a block walks several chunks
constexpr int kOptimMaxGroups = 8;
struct OptimGeom { int32_t chunk, nchunks, per_block, grid; };
DAD_HD inline void optim_block_chunks(const OptimGeom& g, int block, int& lo, int& hi) {
    lo = block * g.per_block;
    hi = lo + g.per_block < g.nchunks ? lo + g.per_block : g.nchunks;
}
// chunk c of a tensor of `numel` elements whose first chunk is `first_chunk`: elements [first, first + count)
DAD_HD inline void optim_chunk_span(const OptimGeom& g, int c, int first_chunk, int64_t numel, int64_t& first, int32_t& count) {
    first = (int64_t)(c - first_chunk) * g.chunk;
    const int64_t left = numel - first;
    count = (int32_t)(left < g.chunk ? left : g.chunk);
}
struct OptimPlan { OptimGeom g{}; std::vector<int32_t> first; };
inline int optim_plan(const int64_t* numel, int n, OptimPlan& p) {
    if (!numel || n <= 0) return fail(DAD_E_INVALID, "optimiser plan: no tensors");
    p.first.assign((size_t)n + 1, 0);
    int64_t chunks = 0;
    for (int t = 0; t < n; ++t) {
        if (numel[t] <= 0) return fail(DAD_E_INVALID, "optimiser plan: tensor %d has numel %lld", t, (long long)numel[t]);
        chunks += (numel[t] + kOptimChunk - 1) / kOptimChunk;
        if (chunks >= INT32_MAX) return fail(DAD_E_INVALID, "optimiser plan: too many elements for one launch");
        p.first[(size_t)t + 1] = (int32_t)chunks;
    }
    p.g.chunk = kOptimChunk;
    p.g.nchunks = (int32_t)chunks;
    p.g.per_block = (p.g.nchunks + kOptimMaxGrid - 1) / kOptimMaxGrid;
    p.g.grid = (p.g.nchunks + p.g.per_block - 1) / p.g.per_block;
    return DAD_OK;
}

// ------------------------------------------------------------------ sampler steps (dad_sampler_step / dad_sampler_loop)
// A reverse step is its dad_sampler_coef.  The ancestral sampler's step at `t`, from the five loaded schedule entries
// at t (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2,
// posterior_log_variance_clipped): the tail kernels' scalars as dad_denoise_step has always formed them.
inline dad_sampler_coef ancestral_coef(int t, float c_recip, float c_recipm1, float coef1, float coef2, float log_var) {
    dad_sampler_coef s{};
    s.t = t;
    s.c_recip = c_recip; s.c_recipm1 = c_recipm1;
    s.coef_x0 = coef1; s.coef_xt = coef2;
    s.guide_x0 = 0.0f;
    s.guide_mean = expf(log_var);
    s.sigma = t == 0 ? 0.0f : expf(0.5f * log_var);
    return s;
}
// Every refusal of steps that come from outside, before anything else is looked at.
inline int check_sampler_steps(const dad_sampler_coef* steps, int n_steps, int n_timesteps) {
    if (n_steps < 1) return fail(DAD_E_INVALID, "n_steps must be positive");
    if (!steps) return fail(DAD_E_INVALID, "null sampler steps");
    for (int i = 0; i < n_steps; ++i) {
        const dad_sampler_coef& s = steps[i];
        if (s.t < 0 || s.t >= n_timesteps)
            return fail(DAD_E_RANGE, "index %d is out of bounds for the schedule of size %d", s.t, n_timesteps);
        const float v[7] = {s.c_recip, s.c_recipm1, s.guide_x0, s.coef_x0, s.coef_xt, s.guide_mean, s.sigma};
        for (float f : v)
            if (!std::isfinite(f)) return fail(DAD_E_INVALID, "sampler step %d: a coefficient is not finite", i);
        if (s.sigma < 0.0f) return fail(DAD_E_INVALID, "sampler step %d: sigma %g is negative", i, (double)s.sigma);
    }
    return DAD_OK;
}
// FNV-1a over bytes: the key of a captured loop hashes what the capture bakes into its launches
inline uint64_t fnv1a_bytes(const void* data, size_t n, uint64_t h = 14695981039346656037ull) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}
static_assert(sizeof(dad_sampler_coef) == 32, "dad_sampler_coef has no padding: its bytes are hashed");
inline uint64_t sampler_steps_hash(const dad_sampler_coef* steps, int n_steps) {
    return fnv1a_bytes(steps, (size_t)n_steps * sizeof(dad_sampler_coef));
}

}  // namespace dadhost
#include "plan_report.hpp"     // the reports travel with the planner: last, since they read everything above
