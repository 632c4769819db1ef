// conv_shapes.hpp — sizing formulas shared by the conv-GEMM kernels (device) and the launch
// planner (host).  No HIP dependency: the planner is also compiled host-only under
// -fsanitize=address,undefined (tests/sanitize/).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define DAD_HD __host__ __device__
#else
#define DAD_HD
#endif

namespace dad {

constexpr int kXSwzPad = 64;    // floats: room for the per-sample slot shifts of the X stage
constexpr size_t kLdsBytes = 160 * 1024;   // LDS of one gfx950 CU

// Rows of the X stage: every sample of the tile with its zero halo, or (layers longer than the tile:
// windowed tiles) BN output positions' worth of input rows of one sample plus the halo on both sides.
DAD_HD inline int conv_xrows(int BN, int Lin, int Lout, int taps) {
    return Lout > BN ? BN * (Lin / Lout) + 2 * (taps / 2) : (BN / Lout) * (Lin + 2 * (taps / 2));
}
// LDS floats of one block (the host sizes the dynamic allocation with the same formula).
// wtaps: weight rows staged per chunk, in taps (taps + 1 when a 1x1 residual conv rides along).
DAD_HD inline size_t conv_lds_floats(int BM, int BN, int KC, int taps, int Lin, int Lout, int SK,
                                     bool bdir = false, int wtaps = 0) {
    const size_t kp = KC + 4;
    const size_t wt = wtaps ? wtaps : taps;
    const size_t stage = (size_t)conv_xrows(BN, Lin, Lout, taps) * kp + kXSwzPad +
                         (bdir ? 0 : wt * BM * kp);
    const size_t epi = (size_t)SK * BN * (BM + 4) + 64;
    const size_t k = 2 * stage;
    return k > epi ? k : epi;
}

// conv_halo8.hpp: the 64 columns of a tile of eight 8-position samples in position-pair-major order.  Column block
// q (16 columns) holds positions {2q, 2q + 1} of all eight samples; MFMA row i of a block (the lane's low four bits
// for the A operand, 4 * (lane / 16) + r for accumulator register r) is:
DAD_HD inline int halo8_sample(int i) { return ((i >> 1) & 1) * 4 + (i >> 2); }
DAD_HD inline int halo8_pos(int i, int q) { return 2 * q + (i & 1); }
// Wave tile tn of the two along N owns blocks {0, 1} / {3, 2} in this order: its block 0 is the tile's outer one, and
// it walks the taps from its outer side (tap index t is conv tap t for tn = 0, 4 - t for tn = 1), so that for every
// wave (tap index 0, block 0) is the product that reads halo rows only.
DAD_HD inline int halo8_block(int tn, int nb) { return tn ? 3 - nb : nb; }
DAD_HD inline int halo8_tap(int tn, int t) { return tn ? 4 - t : t; }
// Lanes that own one (sample, group) pair in that kernel's epilogue — its `lpp`: a pair is 8 positions x cpg channels
// in float4, a thread owns (64 * BM / 4) / threads of them.  A pair of more than 64 lanes spans lpp / 64 waves, whose
// partial sums meet through LDS.
DAD_HD inline int halo8_lanes_per_pair(int BM, int threads, int cpg) { return (8 * (cpg / 4)) / ((64 * BM / 4) / threads); }
// LDS floats of a conv_halo8w_f32 block: its two stages hold the X rows alone (the weights never pass through LDS),
// so the epilogue's exchange tile decides.
DAD_HD inline size_t halo8w_lds_floats(int BM, int SK) { return conv_lds_floats(BM, 64, 32, 5, 8, 8, SK, /*bdir=*/true); }

// conv_wgrad (train_bwd.hpp)
constexpr int WG_THREADS = 512;             // 8 waves: TM x TN wave tiles of 32 x 32 (x TAPS), the rest split K
constexpr int WG_ROWS = 64;                  // G rows per staged chunk: spc = max(1, 64 / Lg) whole samples
constexpr int WG_MAX_GROWS = 128, WG_MAX_ZROWS = 160;      // rows one chunk may stage (registers of chunk_load)

constexpr int COLS_MAX = 120;                // col_sums_many_kernel: arrays per launch (descriptors travel as kernel arguments)

DAD_HD inline int wgrad_segz(int Lz, int taps, int pad) { return Lz + pad + (taps - 1 - pad); }
DAD_HD inline int wgrad_round64(int v) { return (v + 63) / 64 * 64; }
// LDS floats: two stages of a chunk (G rows [spc * Lg][32 TM], Z rows with halo [spc * SEGZ][32 TN], each part
// rounded up to whole 64-float4 wave-instructions of the LDS-DMA), and afterwards the K-group reduction tree, whose
// first round parks half of the block's accumulators: 4 waves x TAPS x 16 x 64.
DAD_HD inline size_t wgrad_lds_floats(int spc, int Lg, int Lz, int taps, int pad, int tm, int tn) {
    const size_t stage = 2 * ((size_t)wgrad_round64(spc * Lg * 8 * tm) * 4 + (size_t)wgrad_round64(spc * wgrad_segz(Lz, taps, pad) * 8 * tn) * 4);
    const size_t red = (size_t)4 * taps * 16 * 64;
    return stage > red ? stage : red;
}

// conv_cc.hpp: rows of a block's X stage — whole samples with their zero halo, or (layers of more than `nr`
// positions: windowed tiles) `nr` rows of one sample plus the halo on both sides.
DAD_HD inline int cc_xrows(int taps, int Lin, int Lout, int nr) {
    return Lout > nr ? nr + 2 * (taps / 2) : (nr / Lout) * (Lin + 2 * (taps / 2));
}

// conv_cc.hpp: 512 threads; a consumer adds up to CC_MAX_SLABS partial slabs per round trip (the BIG forms take two).
constexpr int CC_THREADS = 512;
constexpr int CC_MAX_SLABS = 8;
// LDS floats of one conv_cc block: [X rows][slice + 4] + [weight taps][32][slice + 4], or the
// exchange tile [8 waves][32][36] (+ the ride's) after the K loop.
DAD_HD inline size_t cc_lds_floats(int slice_ch, int taps, int wtaps, int Lin, int Lout, int nr) {
    const size_t xs = slice_ch + 4;
    const size_t k = (size_t)cc_xrows(taps, Lin, Lout, nr) * xs + (size_t)wtaps * 32 * xs;
    const size_t e = (size_t)2 * 8 * nr * 36;
    return k > e ? k : e;
}
// final_cc_kernel: the 1x1 output conv's weights and bias + one sample of final_conv[0]'s output
DAD_HD inline size_t final_cc_lds_floats(int td, int dim, int H) {
    return (size_t)td * dim + ((td + 3) & ~3) + (size_t)H * (dim + 4);
}

// final_posterior_kernel (pointwise.hpp)
constexpr int FINAL_COLS = 32;   // trajectory positions per block (256 blocks at B*H = 8192)
// a block keeps the weight rows of ITS output columns (gy = gridDim.y column groups), the biases and
// the activation tile
DAD_HD inline int final_rows_local(int td, int gy) {
    constexpr int JG = 256 / FINAL_COLS;
    const int col_groups = (td + JG - 1) / JG;
    return (col_groups + gy - 1) / gy * JG;
}
DAD_HD inline size_t final_lds_floats(int td, int dim, int gy) {
    return (size_t)final_rows_local(td, gy) * dim + ((td + 3) & ~3) + (size_t)FINAL_COLS * (dim + 4);
}

// conv_seam.hpp: a block owns 32 rows (32 / H whole samples) and all `dim` output channels, 4 * dim threads.  Its X
// stage holds one 16-channel granule per row (SEAM_KP floats: 16-byte aligned, an odd number of 16-byte slots).
constexpr int SEAM_KP = 20;
DAD_HD constexpr int seam_threads(int dim) { return 4 * dim; }
DAD_HD inline int seam_xf(int H) { return (32 / H) * (H + 4) * SEAM_KP + kXSwzPad; }
// [32][dim + 4] activation / exchange tile | [td][dim] final_conv[1] | bias | X stage | [32][dim + 4] the ride's tile
DAD_HD inline size_t seam_lds_floats(int td, int dim, int H) {
    return (size_t)2 * 32 * (dim + 4) + (size_t)td * dim + ((td + 3) & ~3) + (size_t)seam_xf(H);
}

// conv_gn_pass.hpp: one block of GNP_THREADS threads holds a (sample, group) pair in NPT float4 per thread,
// NPT a power of two up to kGnPassMaxNpt: pairs of up to GNP_THREADS * 4 * kGnPassMaxNpt elements (cpg x L)
constexpr int GNP_THREADS = 256;
constexpr int kGnPassMaxNpt = 32;

// conv_ccw.hpp (wide small-batch convs).  K phase: X rows with halo [XROWS][slice + 4], the additive
// terms [rows][slice + 4], gamma / beta [2][slice], pair statistics; afterwards the exchange tile.
constexpr int kCcwMaxPairs = 64;         // (sample, group) pairs of one block's input slice
DAD_HD inline size_t ccw_lds_floats(int slice_ch, int taps, int Lin, int Lout, int nr) {
    const int spt = nr / Lout;
    const size_t xs = slice_ch + 4;
    const size_t k = (size_t)spt * (Lin + 2 * (taps / 2)) * xs + (size_t)spt * Lin * xs + 2 * (size_t)slice_ch +
                     2 * kCcwMaxPairs;
    const size_t e = (size_t)2 * 8 * nr * 36;
    return k > e ? k : e;
}

// project_kernel<RB, KP> (pointwise.hpp): KP = 16 waves split k; a block keeps RB rows and their KP partial sets
constexpr int PROJ_KP = 16;
DAD_HD inline size_t project_row_lds_bytes(int D) { return (size_t)(1 + PROJ_KP) * D * sizeof(float); }
// project_gemm_kernel (pointwise.hpp)
constexpr int PG_THREADS = 256;
constexpr int PG_KC = 64;                     // k values per staged chunk
constexpr int PG_AS = 33;                     // LDS row stride of the staged v chunk [k][32 rows]
DAD_HD inline size_t project_gemm_lds_floats() { return (size_t)4 * PG_KC * PG_AS + 64; }

// violation_grad.hpp.  Row form, backward: VG_ROW_WAVES waves share the rows of P; a block keeps r_b and g_b.
constexpr int VG_ROW_WAVES = 16;
DAD_HD inline size_t vg_row_bwd_lds_bytes(int D) { return (size_t)2 * D * sizeof(float); }
// GEMM form (PG_THREADS, PG_KC, PG_AS as project_gemm_kernel).  Backward: each wave also stages its P tile
// [32 rows of P][PG_KC k], rows VG_PS floats apart (odd: the transposed reads of the B operand spread over the banks).
constexpr int VG_PS = PG_KC + 1;
DAD_HD inline size_t vg_gemm_bwd_lds_floats() { return (size_t)4 * (PG_KC * PG_AS + 32 * VG_PS); }
constexpr int VG_TAIL_THREADS = 256;          // violation_sum_kernel, violation_scatter_kernel

// guide_mlp.hpp: one block owns GM_ROWS consecutive rows of B * H; every kept tensor is [width][GM_AS] in LDS (the
// row index contiguous: the A operand's layout, odd stride).  The limits of the value nets the library evaluates
// are stated here and nowhere else (plan_guide reads them; the binding and the tests read plan_guide).
constexpr int GM_THREADS = 256;
constexpr int GM_ROWS = 32;
constexpr int GM_AS = 33;
constexpr int GM_MIN_LAYERS = 2, GM_MAX_LAYERS = 4;        // Linear layers, the last one with a single output
constexpr int GM_MAX_WIDTH = 512;                          // hidden units of one layer
DAD_HD inline int guide_pad(int width) { return (width + 31) / 32 * 32; }      // whole 32-column MFMA tiles (and even K)
// LDS floats: the input tile and every hidden activation (later overwritten by its delta), each zero-padded to whole
// tiles; `keeps_derivative` (Mish): act'(a) of every hidden layer as well, since h alone does not give it
DAD_HD inline size_t guide_lds_floats(int in_dim, const int* widths, int n_layers, bool keeps_derivative) {
    size_t cols = (size_t)guide_pad(in_dim);
    for (int i = 0; i + 1 < n_layers; ++i) cols += (size_t)guide_pad(widths[i]) * (keeps_derivative ? 2 : 1);
    return cols * GM_AS;
}

}  // namespace dad
