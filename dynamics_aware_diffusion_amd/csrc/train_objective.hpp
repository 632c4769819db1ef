// train_objective.hpp — the training objective around the denoiser, on the device (gfx950, fp32):
//   * objective head: x_t = q_sample(x_0, t, noise), and after the denoiser the weighted L1 / L2 mean with its unit
//     gradient                                               (m_diffuser/models/diffusion.py:138-157, 253-290)
//   * the time chain per batch row: SinusoidalPosEmb lookup -> Linear -> Mish -> Linear, Mish, and every
//     ResidualTemporalBlock's Linear side by side, forward and backward (temporal_unet.py:19-32, 97-100, 155-160)
// Every GEMM of the chain is one instantiation of time_gemm_kernel: 32 x 32 output tiles on v_mfma_f32_32x32x2_f32,
// the block's four waves take the K chunks round robin and meet in LDS in wave order; operands are staged through
// LDS with zeros outside the matrices, so ragged batches (4, 5, 9, 250 ...) and ragged widths run the same
// instructions on zero-filled edges.  No atomics: every reduction has a fixed order, results are bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dad.h"
#include "conv_gemm.hpp"
#include "train_bwd.hpp"
#include "violation_grad.hpp"

namespace dad {

// ------------------------------------------------------------------------------ objective head
struct ObjectiveParams {
    const float* x0;         // (B, H, td)
    const float* noise;      // (B, H, td)
    const float* weights;    // (B, H, td) or nullptr
    const float* sqrt_ac;    // [T] sqrt_alphas_cumprod
    const float* sqrt_1m_ac; // [T] sqrt_one_minus_alphas_cumprod
    const int32_t* t_in;     // [B] timesteps as drawn
    int32_t* t_rows;         // [B] the same clamped to [0, T-1]: what every table read of the step uses
    int32_t* row_index;      // [B] 0 .. B-1 (row of the time projections sample b reads)
    float* xt;               // (B, H, td) noisy trajectory
    const float* out;        // (B, H, td) denoiser output
    float* partial;          // [nblocks] per-block sums of the weighted elementwise loss
    float* loss;             // device scalar
    const float* d_loss;     // device scalar: autograd's incoming gradient
    float* d_out;            // (B, H, td) d loss / d out
    long n;                  // B * H * td
    int32_t row_elems;       // H * td
    int32_t B, T;
    int32_t l1;              // 1: |d|, 0: d^2
    int32_t predict_epsilon; // target = noise, else x0
    int32_t nblocks;         // blocks of objective_loss_partial_kernel
};
constexpr int OBJ_THREADS = 256;

// x_t = sqrt_ac[t_b] * x0 + sqrt_1m_ac[t_b] * noise with torch's own three roundings (two products, one sum: the
// intrinsics keep the compiler from contracting them into an fma), so x_t equals q_sample's bit for bit.
__global__ __launch_bounds__(OBJ_THREADS) void objective_xt_kernel(const ObjectiveParams p) {
    const long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (i < p.B) {
        p.t_rows[i] = min(max(p.t_in[i], 0), p.T - 1);
        p.row_index[i] = (int32_t)i;
    }
    if (i >= p.n) return;
    const int b = (int)(i / p.row_elems);
    const int t = min(max(p.t_in[b], 0), p.T - 1);
    p.xt[i] = __fadd_rn(__fmul_rn(p.sqrt_ac[t], p.x0[i]), __fmul_rn(p.sqrt_1m_ac[t], p.noise[i]));
}

// sum over a block's 256 values in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ float objective_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = OBJ_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// partial[block] = sum of w * |out - target| (or (out - target)^2) over the block's elements: element i belongs to
// thread i % (nblocks * 256), every thread adds its elements in index order
__global__ __launch_bounds__(OBJ_THREADS) void objective_loss_partial_kernel(const ObjectiveParams p) {
    __shared__ float red[OBJ_THREADS];
    const float* target = p.predict_epsilon ? p.noise : p.x0;
    float acc = 0.0f;
    for (long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x; i < p.n; i += (long)p.nblocks * OBJ_THREADS) {
        const float d = p.out[i] - target[i];
        float v = p.l1 ? fabsf(d) : d * d;
        if (p.weights != nullptr) v *= p.weights[i];
        acc += v;
    }
    const float s = objective_block_sum(acc, red);
    if (threadIdx.x == 0) p.partial[blockIdx.x] = s;
}

// loss = (sum of the partials, in a fixed order) / n
__global__ __launch_bounds__(OBJ_THREADS) void objective_loss_final_kernel(const ObjectiveParams p) {
    __shared__ float red[OBJ_THREADS];
    float acc = 0.0f;
    for (int i = threadIdx.x; i < p.nblocks; i += OBJ_THREADS) acc += p.partial[i];
    const float s = objective_block_sum(acc, red);
    if (threadIdx.x == 0) *p.loss = s / (float)p.n;
}

// d loss / d out = g * sign(d) w / n (L1; sign(0) = 0 as torch defines it) or g * 2 d w / n (L2), g read on the device
__device__ __forceinline__ float objective_unit_grad(const ObjectiveParams& p, long i) {
    const float* target = p.predict_epsilon ? p.noise : p.x0;
    const float d = p.out[i] - target[i];
    float u = p.l1 ? (d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : 0.0f) : 2.0f * d;
    if (p.weights != nullptr) u *= p.weights[i];
    return u;
}
__global__ __launch_bounds__(OBJ_THREADS) void objective_dout_kernel(const ObjectiveParams p) {
    const long i = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
    if (i >= p.n) return;
    const float g = *p.d_loss;
    p.d_out[i] = g * (objective_unit_grad(p, i) / (float)p.n);
}

// ------------------------------------------------------------------------------ dynamics-aware objective
// dad_train_dynamics_objective_forward / _backward: the violation |v - vP|^2 of the predicted plan x0_hat beside the
// objective above, from the same x_t and `out`.  x0_hat is never written: the violation kernels' gather forms
//   v = std * x0_hat + mean,  x0_hat = a_b x_t - c_b out  (a_b = sqrt_recip_ac[t_b], c_b = sqrt_recipm1_ac[t_b]; two
//   products and one difference, each rounded: torch's predict_start_from_noise bit for bit)  or  x0_hat = out,
// t_b as objective_xt_kernel clamped it (ObjectiveParams.t_rows).  The forward kernels are project_kernel's gather,
// mat-vec and violation branch (row form: the same device functions) and violation_fwd_gemm_kernel's body on that gather;
// the backward kernels are the bodies of violation_grad.hpp with the per-trajectory factor
// d_loss * projection_weight * tw[t_b] / (B D) formed on the device and an epilogue that writes d total / d out once:
//   d_out = d_loss * diffusion_weight * u / n + s_b * d_x0hat,   s_b = -c_b, or 1 when the model predicts x_0.
struct DynamicsParams {
    ObjectiveParams obj;         // x_t, out, t_rows, d_loss, d_out, n and what the diffusion term's unit gradient reads
    ViolationFwdParams fwd;      // P, the normaliser, the shape, r (resid), per-trajectory violation or column-block sums
    ViolationBwdParams bwd;      // r, g
    const float* recip;          // [T] sqrt_recip_alphas_cumprod
    const float* recipm1;        // [T] sqrt_recipm1_alphas_cumprod
    const float* tw;             // [T] timestep weights or nullptr (ones)
    float* parts;                // device float[3]: Ld, projection_weight * Lp, total
    float diffusion_weight, projection_weight;
    float bd;                    // B * D
};

// element d of trajectory b of the predicted plan, in physical units (proj_gather on x0_hat)
__device__ __forceinline__ float dynamics_gather(const DynamicsParams& q, int b, int d, int nstate, int td) {
    const ProjParams& p = q.fwd.proj;
    int ts, c;
    float sd, mn;
    if (d < nstate) {
        ts = d / p.n;
        c = d - ts * p.n;
        if (ts >= p.H) ts = p.H - 1;
        sd = p.obs_std[c]; mn = p.obs_mean[c];
    } else {
        const int dd = d - nstate;
        ts = dd / p.m;
        const int k = dd - ts * p.m;
        c = p.od + k;
        sd = p.act_std[k]; mn = p.act_mean[k];
    }
    const long i = ((long)b * p.H + ts) * td + c;
    float x0h = q.obj.out[i];
    if (q.obj.predict_epsilon) {
        const int t = q.obj.t_rows[b];
        x0h = __fsub_rn(__fmul_rn(q.recip[t], q.obj.xt[i]), __fmul_rn(q.recipm1[t], x0h));
    }
    return x0h * sd + mn;
}
// d L / d violation of trajectory b
__device__ __forceinline__ float dynamics_row_weight(const DynamicsParams& q, int b) {
    const float tw = q.tw != nullptr ? q.tw[q.obj.t_rows[b]] : 1.0f;
    return *q.obj.d_loss * (q.projection_weight * tw / q.bd);
}
// d total / d out of element e of trajectory b, `dx`: the projection term's gradient with respect to x0_hat there
__device__ __forceinline__ void dynamics_store_dout(const DynamicsParams& q, int b, int e, float dx) {
    const ObjectiveParams& p = q.obj;
    const long i = (long)b * p.row_elems + e;
    const float s = p.predict_epsilon ? -q.recipm1[p.t_rows[b]] : 1.0f;
    p.d_out[i] = (*p.d_loss * q.diffusion_weight) * (objective_unit_grad(p, i) / (float)p.n) + s * dx;
}

// Row form, forward: project_kernel's two halves (pointwise.hpp: the gather and mat-vec, then the violation branch, r
// kept) on the predicted plan.  One block = RB trajectories.
template <int RB, int KP>
__global__ __launch_bounds__(64 * KP) void dynamics_violation_fwd_row_kernel(const DynamicsParams q) {
    extern __shared__ __attribute__((aligned(16))) float v[];    // [RB][D] rows, then [KP][RB][D] partials
    const ProjParams& p = q.fwd.proj;
    float* part = v + RB * p.D;
    project_rows_matvec<RB, KP>(p, v, part, [&](int b, int d, int nstate, int td) { return dynamics_gather(q, b, d, nstate, td); });
    project_rows_violation<RB, KP>(p, v, part);
}

__global__ __launch_bounds__(PG_THREADS) void dynamics_violation_fwd_gemm_kernel(const DynamicsParams q) {
    extern __shared__ __attribute__((aligned(16))) float vg_sm[];
    violation_fwd_gemm_body(q.fwd, vg_sm, [&](int b, int d, int nstate, int td) { return dynamics_gather(q, b, d, nstate, td); });
}

// parts[1] = projection_weight * sum_b tw[t_b] violation_b / (B D), parts[2] = diffusion_weight * parts[0] + parts[1]
// (parts[0]: objective_loss_final_kernel's, earlier on the stream).  One block; thread i adds trajectories i, i + 256, ...
// in order (gemm form: each one's column-block sums first, in column-block order), then the block's fixed tree.
__global__ __launch_bounds__(OBJ_THREADS) void dynamics_parts_kernel(const DynamicsParams q) {
    __shared__ float red[OBJ_THREADS];
    const int B = q.obj.B, cb = q.fwd.col_blocks;
    float acc = 0.0f;
    for (int b = threadIdx.x; b < B; b += OBJ_THREADS) {
        float viol;
        if (cb > 0) {
            viol = 0.0f;
            for (int c = 0; c < cb; ++c) viol += q.fwd.part[(long)b * cb + c];
        } else {
            viol = q.fwd.proj.violation[b];
        }
        acc += (q.tw != nullptr ? q.tw[q.obj.t_rows[b]] : 1.0f) * viol;
    }
    const float s = objective_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float lp = q.projection_weight * (s / q.bd);
        q.parts[1] = lp;
        q.parts[2] = q.diffusion_weight * q.parts[0] + lp;
    }
}

__global__ __launch_bounds__(64 * VG_ROW_WAVES) void dynamics_violation_bwd_row_kernel(const DynamicsParams q) {
    extern __shared__ __attribute__((aligned(16))) float vg_sm[];
    violation_bwd_row_body(q.bwd, vg_sm, [&](int b) { return dynamics_row_weight(q, b); },
                           [&](int b, int e, float v) { dynamics_store_dout(q, b, e, v); });
}

__global__ __launch_bounds__(PG_THREADS) void dynamics_violation_bwd_gemm_kernel(const DynamicsParams q) {
    extern __shared__ __attribute__((aligned(16))) float vg_sm[];
    violation_bwd_gemm_body(q.bwd, vg_sm, [&](int b) { return dynamics_row_weight(q, b); });
}

// d total / d out from g: one thread per element (violation_scatter_kernel's indexing)
__global__ __launch_bounds__(VG_TAIL_THREADS) void dynamics_scatter_dout_kernel(const DynamicsParams q) {
    const ViolationBwdParams& p = q.bwd;
    const long i = (long)blockIdx.x * VG_TAIL_THREADS + threadIdx.x;
    if (i >= (long)p.B * p.row_elems) return;
    const int b = (int)(i / p.row_elems);
    const int e = (int)(i - (long)b * p.row_elems);
    const int td = p.od + p.m;
    const int ts = e / td, c = e - ts * td;
    dynamics_store_dout(q, b, e, vg_dx_elem(p, p.g + (long)b * p.D, ts, c));
}

// ------------------------------------------------------------------------------ time chain
constexpr int TG_THREADS = 256;
constexpr int TG_KC = 32;              // k values a wave stages per chunk
constexpr int TG_LD = 33;              // LDS row stride of a staged [k][32] operand
constexpr int TG_MAX_BLOCKS = 4 * DAD_MAX_LEVELS;     // ResidualTemporalBlocks of a net: 2 per level down, 2 mid, 2 per level up

// Every block's time_mlp.1 side by side, in launch order: columns [off[k], off[k + 1]) of the projection rows belong
// to block k (padded widths, multiples of 32: a 32-wide tile never straddles two blocks).
struct TimeBlocks {
    const float* w[TG_MAX_BLOCKS];     // (C_k, time_dim) device copies of the weights
    const float* b[TG_MAX_BLOCKS];     // (C_k)
    float* dw[TG_MAX_BLOCKS];          // gradient tensors (backward only)
    float* db[TG_MAX_BLOCKS];
    int32_t off[TG_MAX_BLOCKS + 1];
    int32_t n;
};
__device__ __forceinline__ int time_block_of(const TimeBlocks& tb, int col) {
    int k = 0;
    while (k + 1 < tb.n && tb.off[k + 1] <= col) ++k;
    return k;
}

enum TimeGemm : int {
    TG_FWD_H1,      // h1[b][n]   = b1[n] + sum_e emb[t_b][e] W1[n][e]
    TG_FWD_TEMB,    // temb[b][m] = b3[m] + sum_n mish(h1[b][n]) W3[m][n];  act = mish(temb)
    TG_FWD_ROWS,    // rows[b][c] = bk[c] + sum_m act[b][m] Wk[c][m]            (all blocks)
    TG_BWD_DWK,     // dWk[c][m]  = sum_b dR[b][c] act[b][m];  dbk[c] = sum_b dR[b][c]
    TG_BWD_DACT,    // slab[z][b][m] = sum_{c in slice z} dR[b][c] Wk[c][m]
    TG_BWD_DW3,     // dW3[m][n]  = sum_b dtemb[b][m] mish(h1[b][n]);  db3[m] = sum_b dtemb[b][m]
    TG_BWD_DH1,     // dh1[b][n]  = mish'(h1[b][n]) sum_m dtemb[b][m] W3[m][n]
    TG_BWD_DW1,     // dW1[n][e]  = sum_b dh1[b][n] emb[t_b][e];  db1[n] = sum_b dh1[b][n]
};
struct TimeGemmParams {
    int32_t M, N, K;         // out[M][N] = sum_k A(i, k) B(k, j)
    int32_t kslice;          // k values per blockIdx.z (a multiple of TG_KC)
    const float* a;          // the activation-side operand (h1 / act / dR / dtemb / dh1), row-major, ld = lda
    int32_t lda;
    const float* w;          // the weight-side operand (W1 / W3) or the second activation (act / h1), ld = ldw
    int32_t ldw;
    const float* emb;        // [T][E] sinusoid table
    const int32_t* t_rows;   // [B] clamped timesteps
    const float* bias;       // forward: bias of the Linear
    const float* h1;         // TG_BWD_DH1: pre-activation whose mish' scales the result
    float* out;              // ld = N (TG_BWD_DACT: slabs of M * N)
    float* out2;             // TG_FWD_TEMB: act; weight gradients: the bias gradient
    TimeBlocks tb;
};

// 0: operand read with k fastest across lanes, 1: with the tile's own index (i or j) fastest — whichever is contiguous
// in memory
template <int MODE> struct TimeGemmOrder {
    static constexpr bool fwd = MODE == TG_FWD_H1 || MODE == TG_FWD_TEMB || MODE == TG_FWD_ROWS;
    static constexpr bool wgrad = MODE == TG_BWD_DWK || MODE == TG_BWD_DW3 || MODE == TG_BWD_DW1;
    static constexpr bool a_tile_fast = wgrad;
    static constexpr bool b_tile_fast = !fwd;
};

template <int MODE>
__device__ __forceinline__ float time_gemm_a(const TimeGemmParams& p, int i, int k) {
    if constexpr (MODE == TG_FWD_H1) return p.emb[(long)p.t_rows[i] * p.K + k];
    else if constexpr (MODE == TG_FWD_TEMB) return mish_f32(p.a[(long)i * p.lda + k]);
    else if constexpr (MODE == TG_FWD_ROWS || MODE == TG_BWD_DACT || MODE == TG_BWD_DH1) return p.a[(long)i * p.lda + k];
    else return p.a[(long)k * p.lda + i];                 // weight gradients: A(i, k = b) = G[b][i]
}
// `blk`: the ResidualTemporalBlock the tile (TG_FWD_ROWS: column j, TG_BWD_DACT: row k) lies in
template <int MODE>
__device__ __forceinline__ float time_gemm_b(const TimeGemmParams& p, int k, int j, int blk) {
    if constexpr (MODE == TG_FWD_H1 || MODE == TG_FWD_TEMB) return p.w[(long)j * p.ldw + k];
    else if constexpr (MODE == TG_FWD_ROWS) return p.tb.w[blk][(long)(j - p.tb.off[blk]) * p.K + k];
    else if constexpr (MODE == TG_BWD_DWK) return p.w[(long)k * p.ldw + j];
    else if constexpr (MODE == TG_BWD_DACT) return p.tb.w[blk][(long)(k - p.tb.off[blk]) * p.N + j];
    else if constexpr (MODE == TG_BWD_DW3) return mish_f32(p.w[(long)k * p.ldw + j]);
    else if constexpr (MODE == TG_BWD_DH1) return p.w[(long)k * p.ldw + j];
    else return p.emb[(long)p.t_rows[k] * p.N + j];       // TG_BWD_DW1
}

// grid = (ceil(M / 32), ceil(N / 32), K slices), 256 threads
template <int MODE>
__global__ __launch_bounds__(TG_THREADS) void time_gemm_kernel(const TimeGemmParams p) {
    __shared__ float sm[4 * 2 * TG_KC * TG_LD];
    using Order = TimeGemmOrder<MODE>;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int i0 = blockIdx.x * 32, j0 = blockIdx.y * 32;
    const int kbeg = blockIdx.z * p.kslice, kend = min(p.K, kbeg + p.kslice);
    float* const As = sm + wave * (2 * TG_KC * TG_LD);    // this wave's [32 k][32 i (+1)]
    float* const Bs = As + TG_KC * TG_LD;                 //             [32 k][32 j (+1)]
    int blk = 0;
    if constexpr (MODE == TG_FWD_ROWS) blk = time_block_of(p.tb, j0);
    if constexpr (MODE == TG_BWD_DWK) blk = time_block_of(p.tb, i0);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nchunks = (kend - kbeg + TG_KC - 1) / TG_KC;
    for (int ch = wave; ch < nchunks; ch += 4) {
        const int k0 = kbeg + ch * TG_KC;
        if constexpr (MODE == TG_BWD_DACT) blk = time_block_of(p.tb, k0);
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            {
                const int kk = Order::a_tile_fast ? 2 * it + h : l32;
                const int ii = Order::a_tile_fast ? l32 : 2 * it + h;
                const int i = i0 + ii, k = k0 + kk;
                As[kk * TG_LD + ii] = (i < p.M && k < kend) ? time_gemm_a<MODE>(p, i, k) : 0.0f;
            }
            {
                const int kk = Order::b_tile_fast ? 2 * it + h : l32;
                const int jj = Order::b_tile_fast ? l32 : 2 * it + h;
                const int j = j0 + jj, k = k0 + kk;
                Bs[kk * TG_LD + jj] = (j < p.N && k < kend) ? time_gemm_b<MODE>(p, k, j, blk) : 0.0f;
            }
        }
        // (wave-private tiles: the wave's own LDS writes are ordered before its reads; no block barrier in the K loop)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < TG_KC / 2; ++q)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * q + h) * TG_LD + l32], Bs[(2 * q + h) * TG_LD + l32], acc, 0, 0, 0);
        // (... and its reads before the next chunk's writes)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    float* const E = sm;                                  // [4 waves][32 rows][33]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        E[(wave * 32 + row) * TG_LD + l32] = acc[r];
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += TG_THREADS) {
        const int r = e >> 5, c = e & 31;
        const int i = i0 + r, j = j0 + c;
        if (i >= p.M || j >= p.N) continue;
        const float v = ((E[r * TG_LD + c] + E[(32 + r) * TG_LD + c]) + E[(64 + r) * TG_LD + c]) + E[(96 + r) * TG_LD + c];
        if constexpr (MODE == TG_FWD_H1) p.out[(long)i * p.N + j] = v + p.bias[j];
        else if constexpr (MODE == TG_FWD_TEMB) {
            const float t = v + p.bias[j];
            p.out[(long)i * p.N + j] = t;
            p.out2[(long)i * p.N + j] = mish_f32(t);
        }
        else if constexpr (MODE == TG_FWD_ROWS) p.out[(long)i * p.N + j] = v + p.tb.b[blk][j - p.tb.off[blk]];
        else if constexpr (MODE == TG_BWD_DWK) p.tb.dw[blk][(long)(i - p.tb.off[blk]) * p.N + j] = v;
        else if constexpr (MODE == TG_BWD_DACT) p.out[((long)blockIdx.z * p.M + i) * p.N + j] = v;
        else if constexpr (MODE == TG_BWD_DH1) p.out[(long)i * p.N + j] = v * mish_grad_f32(p.h1[(long)i * p.N + j]);
        else p.out[(long)i * p.N + j] = v;
    }
    if constexpr (Order::wgrad) {
        // the bias gradient of the tile's 32 rows: the column sums of G over the batch, by the blocks of the first
        // tile column — thread (col, rg) adds batch rows rg, rg + 8, ..., the eight partials are added in group order
        if (blockIdx.y != 0) return;
        __syncthreads();
        const int col = tid & 31, rg = tid >> 5;
        const int i = i0 + col;
        float s = 0.0f;
        if (i < p.M)
            for (int b = rg; b < p.K; b += 8) s += p.a[(long)b * p.lda + i];
        sm[rg * TG_LD + col] = s;
        __syncthreads();
        if (rg == 0 && i < p.M) {
            float v = sm[col];
#pragma unroll
            for (int k = 1; k < 8; ++k) v += sm[k * TG_LD + col];
            if constexpr (MODE == TG_BWD_DWK) p.tb.db[blk][i - p.tb.off[blk]] = v;
            else p.out2[i] = v;
        }
    }
}

// d act = sum of the K slabs in slice order; d temb = d act * mish'(temb)
__global__ __launch_bounds__(256) void time_dtemb_kernel(float* dtemb, const float* slab, const float* temb, long n, int ks) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = slab[i];
    for (int k = 1; k < ks; ++k) v += slab[(long)k * n + i];
    // act = mish(temb): d temb = d act * mish'(temb)
    dtemb[i] = v * mish_grad_f32(temb[i]);
}

}  // namespace dad
