// violation_grad.hpp — the dynamics violation viol_b = |v_b - v_b P|^2 as a differentiable pair
// (dad_projection_violation_fwd / _bwd; losses/__init__.py:161-186 under torch autograd).  gfx950.
//
// Forward keeps the residual r = v - vP, (B, D) fp32, in the caller's workspace; backward reads it:
//   g_b = 2 w_b (r_b - r_b P^T),  d_x = the transpose of proj_gather's gather + de-normalisation applied to g
// (the last state is gathered twice, so its two entries of g add; observation channels beyond the state get 0).
// P is read as it is: neither symmetric nor idempotent to this code.
//
// Two forms, chosen by plan_violation_grad (host_plan.hpp):
//   row   forward: project_kernel's violation branch with ProjParams.resid set (pointwise.hpp);
//         backward: violation_bwd_row_kernel, one trajectory per block.  (r P^T)_d = P[d,:] . r_b is a dot
//         product along a row of P: a wave reads it 256 contiguous bytes at a time and adds its 64 lanes in a
//         shuffle tree.
//   gemm  32 trajectories x 32 columns per block on v_mfma_f32_32x32x2_f32, four waves splitting K in chunks of
//         PG_KC and meeting in LDS in fixed order, as project_gemm_kernel.  Forward: the B operand is P, read as
//         there; per-(trajectory, column block) sums of r^2 go to the workspace and violation_sum_kernel adds them
//         in column-block order.  Backward: the B operand is P^T — lane (column d, k half) wants P[d][k], which
//         along the lanes is a stride of D floats; so each wave stages its [32 rows of P][PG_KC] tile coalesced
//         (lane = k: 256 contiguous bytes per row) into LDS, rows VG_PS = PG_KC + 1 floats apart, and reads it
//         transposed.  g goes to the workspace; violation_scatter_kernel writes d_x from it (the two entries of
//         the last state lie in different column blocks).
// No atomics anywhere: every sum has one order, the same inputs give the same bits.
//
// The three kernels written here are thin __global__ wrappers over *_body templates, which state the arithmetic once:
// the dynamics-aware objective (train_objective.hpp) instantiates the same bodies with another gather (x0_hat formed
// from x_t and the denoiser's output), another per-trajectory weight and another store (d total / d out).
#pragma once
#include "pointwise.hpp"

namespace dad {

struct ViolationFwdParams {
    ProjParams proj;         // x, P, the normaliser, violation (B) and resid (B, D)
    float* part;             // (B, col_blocks) sums of r^2 over one column block
    int32_t col_blocks;
};

struct ViolationBwdParams {
    const float* P;          // [D][D]
    const float* obs_std; const float* act_std;
    const float* r;          // (B, D) residual of the forward pass
    const float* w;          // (B) d L / d violation
    float* g;                // gemm form: (B, D)
    float* dx;               // (B, H, od + m), fully overwritten
    int32_t B, H, n, od, m, D;
    int32_t row_elems;       // H (od + m)
};

// d_x[ts][c] of one trajectory from its g (LDS or global)
__device__ __forceinline__ float vg_dx_elem(const ViolationBwdParams& p, const float* g, int ts, int c) {
    if (c < p.n) {
        float s = g[ts * p.n + c];
        if (ts == p.H - 1) s += g[p.H * p.n + c];
        return p.obs_std[c] * s;
    }
    if (c < p.od) return 0.0f;
    const int k = c - p.od;
    return p.act_std[k] * g[(p.H + 1) * p.n + ts * p.m + k];
}

// ------------------------------------------------------------------------------------------ row form, backward
// One block = one trajectory, VG_ROW_WAVES waves.  Wave q owns rows d = q, q + 16, ... of P, four at a time (four
// independent streams of loads in flight); LDS: r_b [D], g_b [D].
// `weight(b)`: d L / d violation of trajectory b; `store(b, e, v)`: what becomes of element e of its d_x.
template <class Weight, class Store>
__device__ __forceinline__ void violation_bwd_row_body(const ViolationBwdParams& p, float* vg_sm, const Weight& weight, const Store& store) {
    const int D = p.D, b = blockIdx.x;
    float* const rs = vg_sm;
    float* const gs = vg_sm + D;
    const float* rb = p.r + (long)b * D;
    for (int k = threadIdx.x; k < D; k += blockDim.x) rs[k] = rb[k];
    __syncthreads();
    const float w2 = 2.0f * weight(b);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int d = wave; d < D; d += 4 * VG_ROW_WAVES) {
        const float* prow[4];
        float acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            prow[u] = p.P + (long)min(d + u * VG_ROW_WAVES, D - 1) * D;      // (rows past D: read row D-1, dropped)
            acc[u] = 0.0f;
        }
        for (int k = lane; k < D; k += 64) {
            const float rk = rs[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fmaf(prow[u][k], rk, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            for (int o = 32; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o, 64);
            const int du = d + u * VG_ROW_WAVES;
            if (lane == 0 && du < D) gs[du] = w2 * (rs[du] - acc[u]);
        }
    }
    __syncthreads();
    const int td = p.od + p.m;
    for (int e = threadIdx.x; e < p.row_elems; e += blockDim.x) {
        const int ts = e / td, c = e - ts * td;
        store(b, e, vg_dx_elem(p, gs, ts, c));
    }
}
__global__ __launch_bounds__(64 * VG_ROW_WAVES) void violation_bwd_row_kernel(const ViolationBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float vg_sm[];
    violation_bwd_row_body(p, vg_sm, [&](int b) { return p.w[b]; },
                           [&](int b, int e, float v) { p.dx[(long)b * p.row_elems + e] = v; });
}

// ------------------------------------------------------------------------------------------ gemm form, forward
// project_gemm_kernel's K loop; the epilogue keeps r = v - vP and the sum of r^2 over this block's 32 columns, per
// trajectory (a row of the tile is 32 consecutive lanes: a shuffle tree inside the half wave).
// `gather(b, d, nstate, td)`: element d of trajectory b in physical units.
template <class Gather>
__device__ __forceinline__ void violation_fwd_gemm_body(const ViolationFwdParams& q, float* vg_sm, const Gather& gather) {
    const ProjParams& p = q.proj;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int D = p.D, H = p.H, td = p.od + p.m;
    const int nstate = (H + 1) * p.n;
    const int b0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    float* const As = vg_sm + wave * (PG_KC * PG_AS);       // this wave's [64 k][32 rows (+1)]
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nchunks = (D + PG_KC - 1) / PG_KC;
    const int dcol = min(d0 + l32, D - 1);                  // (columns past D read column D-1 and are dropped)
    for (int ch = wave; ch < nchunks; ch += 4) {
        const int k0 = ch * PG_KC;
        float bv[PG_KC / 2];
#pragma unroll
        for (int j = 0; j < PG_KC / 2; ++j) {
            const int k = min(k0 + 2 * j + h, D - 1);       // (rows past D: masked by the zero A operand)
            bv[j] = p.P[(long)k * D + dcol];
        }
        {
            const int k = k0 + lane;
            for (int r = 0; r < 32; ++r) {
                const int b = b0 + r;
                float v = 0.0f;
                if (k < D && b < p.B) v = gather(b, k, nstate, td);
                As[lane * PG_AS + r] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (wave-private tile, as project_gemm_kernel)
#pragma unroll
        for (int j = 0; j < PG_KC / 2; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * j + h) * PG_AS + l32], bv[j], acc, 0, 0, 0);
    }
    __syncthreads();
    float* const E = vg_sm;                                 // [4 waves][32 rows][33]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        E[(wave * 32 + row) * PG_AS + l32] = acc[r];
    }
    __syncthreads();
    // 1024 outputs over 256 threads: every thread takes part in all four rounds (the shuffles are wave-wide)
    for (int e = tid; e < 32 * 32; e += PG_THREADS) {
        const int r = e >> 5, cidx = e & 31;
        const int b = b0 + r, d = d0 + cidx;
        float diff = 0.0f;
        if (b < p.B && d < D) {
            const float proj = ((E[r * PG_AS + cidx] + E[(32 + r) * PG_AS + cidx]) + E[(64 + r) * PG_AS + cidx]) +
                               E[(96 + r) * PG_AS + cidx];
            diff = gather(b, d, nstate, td) - proj;
            p.resid[(long)b * D + d] = diff;
        }
        float sq = diff * diff;
        for (int o = 16; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        if (cidx == 0 && b < p.B) q.part[(long)b * q.col_blocks + blockIdx.y] = sq;
    }
}
__global__ __launch_bounds__(PG_THREADS) void violation_fwd_gemm_kernel(const ViolationFwdParams q) {
    extern __shared__ __attribute__((aligned(16))) float vg_sm[];
    const ProjParams& p = q.proj;
    violation_fwd_gemm_body(q, vg_sm, [&](int b, int d, int nstate, int td) {
        return proj_gather(p, p.x + (long)b * p.H * td, d, nstate, td);
    });
}

// violation[b] = the column blocks' partial sums, added in column-block order
__global__ __launch_bounds__(VG_TAIL_THREADS) void violation_sum_kernel(const float* part, float* violation, int B,
                                                                        int col_blocks) {
    const int b = blockIdx.x * VG_TAIL_THREADS + threadIdx.x;
    if (b >= B) return;
    const float* pb = part + (long)b * col_blocks;
    float acc = 0.0f;
    for (int c = 0; c < col_blocks; ++c) acc += pb[c];
    violation[b] = acc;
}

// ------------------------------------------------------------------------------------------ gemm form, backward
// C[b][d] = sum_k r[b][k] P[d][k] for 32 trajectories x 32 rows d of P; g[b][d] = 2 w_b (r[b][d] - C[b][d]).
template <class Weight>
__device__ __forceinline__ void violation_bwd_gemm_body(const ViolationBwdParams& p, float* vg_sm, const Weight& weight) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int D = p.D;
    const int b0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    float* const As = vg_sm + wave * (PG_KC * PG_AS + 32 * VG_PS);      // this wave's r chunk [64 k][32 rows (+1)]
    float* const Ps = As + PG_KC * PG_AS;                               //   and P tile [32 rows d][64 k (+1)]
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nchunks = (D + PG_KC - 1) / PG_KC;
    for (int ch = wave; ch < nchunks; ch += 4) {
        const int k = ch * PG_KC + lane;
        const bool kin = k < D;                             // (k past D: both operands zero)
        float pv[32], rv[32];
#pragma unroll
        for (int dd = 0; dd < 32; ++dd) {
            const int drow = min(d0 + dd, D - 1);           // (rows past D read row D-1 and are dropped)
            pv[dd] = kin ? p.P[(long)drow * D + k] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 32; ++r) rv[r] = (kin && b0 + r < p.B) ? p.r[(long)(b0 + r) * D + k] : 0.0f;
#pragma unroll
        for (int dd = 0; dd < 32; ++dd) Ps[dd * VG_PS + lane] = pv[dd];
#pragma unroll
        for (int r = 0; r < 32; ++r) As[lane * PG_AS + r] = rv[r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // (wave-private tiles, as project_gemm_kernel)
#pragma unroll
        for (int j = 0; j < PG_KC / 2; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * j + h) * PG_AS + l32], Ps[l32 * VG_PS + 2 * j + h], acc, 0, 0, 0);
    }
    __syncthreads();
    float* const E = vg_sm;                                 // [4 waves][32 rows][33]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        E[(wave * 32 + row) * PG_AS + l32] = acc[r];
    }
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += PG_THREADS) {
        const int r = e >> 5, cidx = e & 31;
        const int b = b0 + r, d = d0 + cidx;
        if (b >= p.B || d >= D) continue;
        const float c = ((E[r * PG_AS + cidx] + E[(32 + r) * PG_AS + cidx]) + E[(64 + r) * PG_AS + cidx]) +
                        E[(96 + r) * PG_AS + cidx];
        p.g[(long)b * D + d] = (2.0f * weight(b)) * (p.r[(long)b * D + d] - c);
    }
}
__global__ __launch_bounds__(PG_THREADS) void violation_bwd_gemm_kernel(const ViolationBwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float vg_sm[];
    violation_bwd_gemm_body(p, vg_sm, [&](int b) { return p.w[b]; });
}

// d_x from g: one thread per element of d_x
__global__ __launch_bounds__(VG_TAIL_THREADS) void violation_scatter_kernel(const ViolationBwdParams p) {
    const long i = (long)blockIdx.x * VG_TAIL_THREADS + threadIdx.x;
    if (i >= (long)p.B * p.row_elems) return;
    const int b = (int)(i / p.row_elems);
    const int e = (int)(i - (long)b * p.row_elems);
    const int td = p.od + p.m;
    const int ts = e / td, c = e - ts * td;
    p.dx[i] = vg_dx_elem(p, p.g + (long)b * p.D, ts, c);
}

}  // namespace dad
