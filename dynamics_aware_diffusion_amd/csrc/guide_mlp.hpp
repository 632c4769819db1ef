// guide_mlp.hpp — a value guide evaluated by the library: the gradient of sum_l V(obs_{b,l}) with respect to x, V a
// small MLP on each horizon step's observation (guides/policies.py:243-271, differentiated as :87-97 does with
// autograd).  The gradient is independent per row (b, l): the MLP's input gradient on the observation channels,
// zero on the rest.
//
// One block = GM_ROWS = 32 consecutive rows of B * H, 4 waves.  Per row
//   forward   h_0 = x[row, :in_dim],  a_i = W_i h_{i-1} + b_i,  h_i = act(a_i),  V = w_L . h_{L-1} + b_L
//   backward  d_{L-1} = w_L * act'(a_{L-1}),  d_{i-1} = (W_i^T d_i) * act'(a_{i-1}),  grad = W_1^T d_1
// The hidden layers run in both directions as v_mfma_f32_32x32x2_f32 GEMMs (exact fp32: a k-ordered fma chain), as
// project_gemm_kernel does: the 32 rows are the MFMA's rows, the waves split the 32-column tiles of the output, the
// weights go from global memory (L2) straight into the B operand — forward from the transposed image [K][N],
// backward from the natural one [N][K], so that a half wave always reads 128 contiguous bytes.  Every kept tensor
// lives in LDS as [column][GM_AS] with the row index contiguous (the A operand's layout; the odd stride keeps the
// accumulator's transposed store and the operand reads conflict-free).  h_i stays between the passes and is overwritten
// in place by d_i: act' comes from h itself (Tanh: 1 - h^2, ReLU: h > 0) or, for Mish, from a second kept tensor.
// The last layer (one output) and its backward product are VALU work, eight lanes per row.
// All widths are zero-padded to whole tiles by the caller (dad_guide_args): padded weights and biases are zero and
// all three activations map 0 to 0, so the padding computes zeros and no loop has a tail.
// No atomics, one writer per element, fixed summation order: the same inputs give the same bits.
// (GM_THREADS, GM_ROWS, GM_AS, guide_pad, guide_lds_floats: conv_shapes.hpp; the launch: plan_guide, host_plan.hpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_gemm.hpp"   // f32x16, mish_fast_f32
#include "train_bwd.hpp"   // mish_grad_f32

namespace dad {

struct GuideParams {
    const float* x;            // (rows, td)
    float* grad;               // (rows, td), fully overwritten
    float* value_rows;         // (rows) or nullptr
    const float* wf[GM_MAX_LAYERS - 1];     // hidden layer i: W^T, [pad[i]][pad[i + 1]]
    const float* wb[GM_MAX_LAYERS - 1];     //                 W,   [pad[i + 1]][pad[i]]
    const float* bias[GM_MAX_LAYERS - 1];   //                 [pad[i + 1]]
    const float* w_last;       // [pad[hidden]]
    const float* b_last;       // one float
    int32_t rows, td, in_dim;
    int32_t hidden;            // hidden layers: n_layers - 1, 1 .. 3
    int32_t pad[GM_MAX_LAYERS];   // pad[0]: the input, pad[i]: hidden layer i (multiples of 32)
};

constexpr int GUIDE_TANH = 0, GUIDE_RELU = 1, GUIDE_MISH = 2;      // DAD_GD_ACTS (static_assert in dad_lib.hip)

template <int ACT>
__device__ __forceinline__ float guide_act(float a) {
    if constexpr (ACT == GUIDE_TANH) return tanhf(a);
    else if constexpr (ACT == GUIDE_RELU) return fmaxf(a, 0.0f);
    else return mish_fast_f32(a);
}
// act'(a) from h = act(a) (Tanh, ReLU); Mish reads the derivative it kept
template <int ACT>
__device__ __forceinline__ float guide_act_grad(float h, float kept) {
    if constexpr (ACT == GUIDE_TANH) return fmaf(-h, h, 1.0f);
    else if constexpr (ACT == GUIDE_RELU) return h > 0.0f ? 1.0f : 0.0f;
    else return kept;
}

// acc (32 rows x 32 columns n0 ..) = A (LDS, [K][GM_AS], K a multiple of 32) x B (global, [K][ldb], columns n0 ..)
__device__ __forceinline__ f32x16 guide_tile(const float* As, const float* Bg, int K, int ldb, int n0, int l32, int h) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float* bcol = Bg + n0 + l32;
    for (int k0 = 0; k0 < K; k0 += 32) {
        float bv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) bv[j] = bcol[(long)(k0 + 2 * j + h) * ldb];
#pragma unroll
        for (int j = 0; j < 16; ++j)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(k0 + 2 * j + h) * GM_AS + l32], bv[j], acc, 0, 0, 0);
    }
    return acc;
}

template <int ACT>
__global__ __launch_bounds__(GM_THREADS) void guide_mlp_kernel(const GuideParams p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const int td = p.td, in_dim = p.in_dim, L = p.hidden;
    const long row0 = (long)blockIdx.x * GM_ROWS;

    // LDS: layer 0 the input tile, layer i hidden layer i (h_i, later d_i), then for Mish act'(a_i) of the hidden
    // layers in the same order.  (Offsets by selects, not by a table: a runtime-indexed local array would be scratch.)
    const int o1 = p.pad[0], o2 = o1 + p.pad[1], o3 = o2 + p.pad[2], o4 = o3 + p.pad[3];      // (unused layers: 0)
    const auto hof = [&](int i) { return sm + GM_AS * (i == 0 ? 0 : i == 1 ? o1 : i == 2 ? o2 : o3); };
    const auto dof = [&](int i) { return hof(i) + GM_AS * (o4 - o1); };
    const auto padof = [&](int i) { return i == 0 ? p.pad[0] : i == 1 ? p.pad[1] : i == 2 ? p.pad[2] : p.pad[3]; };
    const auto layer = [&](const float* const* a, int i) { return i == 0 ? a[0] : i == 1 ? a[1] : a[2]; };
    float* const H0 = sm;

    // h_0: the observation channels of the block's rows, zero beyond in_dim and beyond the last row
    for (int e = tid; e < GM_ROWS * o1; e += GM_THREADS) {
        const int r = e / o1, k = e - r * o1;
        float v = 0.0f;
        if (k < in_dim && row0 + r < p.rows) v = p.x[(row0 + r) * td + k];
        H0[k * GM_AS + r] = v;
    }
    // the channels the guide does not read get no gradient
    if (td > in_dim) {
        const int extra = td - in_dim;
        for (int e = tid; e < GM_ROWS * extra; e += GM_THREADS) {
            const int r = e / extra, k = e - r * extra;
            if (row0 + r < p.rows) p.grad[(row0 + r) * td + in_dim + k] = 0.0f;
        }
    }
    __syncthreads();

    // ---- forward: hidden layer i from layer i - 1 ----
    for (int i = 1; i <= L; ++i) {
        const int K = padof(i - 1), N = padof(i);
        const float* const src = hof(i - 1);
        const float* const wt = layer(p.wf, i - 1);
        const float* const bs = layer(p.bias, i - 1);
        for (int n0 = wave * 32; n0 < N; n0 += 4 * 32) {
            const f32x16 acc = guide_tile(src, wt, K, N, n0, l32, h);
            const float b = bs[n0 + l32];
            float* hc = hof(i) + (n0 + l32) * GM_AS;
            float* dc = dof(i) + (n0 + l32) * GM_AS;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float a = acc[r] + b;
                hc[row] = guide_act<ACT>(a);
                if constexpr (ACT == GUIDE_MISH) dc[row] = mish_grad_f32(a);
            }
        }
        __syncthreads();
    }

    // ---- the last layer and its backward product: V = w_L . h_L + b_L,  d_L = w_L * act'(a_L), in place ----
    {
        const int r = tid >> 3, s = tid & 7;
        const int N = padof(L);
        float* const HL = hof(L);
        const float* const DL = dof(L);
        float v = 0.0f;
        for (int k = s; k < N; k += 8) {
            const float w = p.w_last[k];
            const float hv = HL[k * GM_AS + r];
            float kept = 0.0f;
            if constexpr (ACT == GUIDE_MISH) kept = DL[k * GM_AS + r];
            v = fmaf(w, hv, v);
            HL[k * GM_AS + r] = w * guide_act_grad<ACT>(hv, kept);
        }
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 1, 64);
        if (p.value_rows != nullptr && s == 0 && row0 + r < p.rows) p.value_rows[row0 + r] = v + p.b_last[0];
    }
    __syncthreads();

    // ---- backward: d_{i-1} = (d_i W_i) * act'(a_{i-1}), in place over h_{i-1} ----
    for (int i = L; i >= 2; --i) {
        const int K = padof(i), N = padof(i - 1);
        const float* const src = hof(i);
        const float* const w = layer(p.wb, i - 1);
        for (int n0 = wave * 32; n0 < N; n0 += 4 * 32) {
            const f32x16 acc = guide_tile(src, w, K, N, n0, l32, h);
            float* hc = hof(i - 1) + (n0 + l32) * GM_AS;
            const float* dc = dof(i - 1) + (n0 + l32) * GM_AS;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                float kept = 0.0f;
                if constexpr (ACT == GUIDE_MISH) kept = dc[row];
                hc[row] = acc[r] * guide_act_grad<ACT>(hc[row], kept);
            }
        }
        __syncthreads();
    }

    // ---- grad[row, :in_dim] = d_1 W_1 ----
    {
        const int K = p.pad[1], N = o1;
        for (int n0 = wave * 32; n0 < N; n0 += 4 * 32) {
            if (n0 >= in_dim) break;                       // (a whole tile of padding)
            const f32x16 acc = guide_tile(hof(1), p.wb[0], K, N, n0, l32, h);
            const int c = n0 + l32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (c < in_dim && row < p.rows) p.grad[row * td + c] = acc[r];
            }
        }
    }
}

}  // namespace dad
