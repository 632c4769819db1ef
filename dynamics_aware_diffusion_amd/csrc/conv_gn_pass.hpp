// conv_gn_pass.hpp — the Conv1dBlock tail (GroupNorm(8) -> Mish -> + time embedding -> + residual,
// temporal_unet.py:57-76 / :106-122) of a layer whose conv ran on windowed tiles (conv_gemm.hpp, WIN):
// layers longer than any tile (horizons 256 / 512), where a (sample, group) pair spans several tiles.
//
// One block per (sample, group) pair.  The conv left conv + bias in `src`; the block holds the whole pair in
// registers (NPT float4 per thread, 4 channels x 1 position each), reduces the mean, then the centred sum of
// squares (two passes over the registers, fp32, fixed order: per-thread sums in index order, a xor butterfly
// inside the wave, the four wave sums in wave order), and writes the activated pair to `dst` (which may be
// `src`: every element is read and written by the same thread).  PADDED semantics as the fused epilogue: rows
// at or beyond `lreal` and channels at or beyond `cpg_real` of a group stay out of the statistics, the padded
// rows are stored as zeros.  Training forward: `stats` receives (mean, rstd) per pair; the conv wrote its
// output into the pre-activation buffer, which is `src` here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_gemm.hpp"   // mish_fast_f32

namespace dad {

struct GnPassParams {
    const float* src;    // [B*L][C] conv + bias
    float* dst;          // [B*L][C] activated output (may equal src)
    const float* gamma;  // [C]
    const float* beta;   // [C]
    const float* temb;   // [C] time-embedding projection, or nullptr
    const int32_t* trow; // per-sample timesteps or nullptr: sample b reads temb + trow[b] * temb_stride
    int32_t temb_stride;
    const float* res;    // [B*L][C] residual, or nullptr
    float* stats;        // [B][8][2] (mean, rstd), or nullptr
    int32_t C, L;        // channels, positions per sample
    int32_t cpg;         // channels per group (C / 8), a multiple of 4
    int32_t lreal;       // > 0: positions of a sample that exist (zero-padded horizon); 0: all
    int32_t cpg_real;    // > 0: channels of a group that exist (zero-padded widths); 0: all
};

// (GNP_THREADS, kGnPassMaxNpt: conv_shapes.hpp)

__device__ __forceinline__ float gnp_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                   // `red` may still be read by the previous reduction
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int NPT>
__global__ __launch_bounds__(GNP_THREADS) void gn_pass_kernel(const GnPassParams p) {
    static_assert(GNP_THREADS == 256, "four waves");
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int cq = p.cpg >> 2;                         // float4 per row of the pair
    const int cq_sh = 31 - __clz(cq);
    const int n4 = cq * p.L;
    const long base = (long)b * p.L * p.C + (long)g * p.cpg;
    const int lr = p.lreal > 0 ? p.lreal : p.L;
    const int creal = p.cpg_real > 0 ? p.cpg_real : p.cpg;
    const float inv_cnt = 1.0f / (float)(lr * creal);

    float4 v[NPT];
    long off[NPT];
    int row[NPT], cl[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int j = tid + k * GNP_THREADS;
        row[k] = j >> cq_sh;
        cl[k] = (j & (cq - 1)) * 4;                    // channel of the float4 inside its group
        off[k] = j < n4 ? base + (long)row[k] * p.C + cl[k] : -1;
        v[k] = off[k] >= 0 ? *reinterpret_cast<const float4*>(p.src + off[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // padded positions hold conv + bias of the edge rows (not zero): out of both passes; padded channels hold
    // exactly zero: nothing for the sum, masked in the variance
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < NPT; ++k)
        if (off[k] >= 0 && row[k] < lr) s += (v[k].x + v[k].y) + (v[k].z + v[k].w);
    const float mean = gnp_block_sum(s, red) * inv_cnt;
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const bool on = off[k] >= 0 && row[k] < lr;
        const float d0 = (on && cl[k] + 0 < creal) ? v[k].x - mean : 0.0f;
        const float d1 = (on && cl[k] + 1 < creal) ? v[k].y - mean : 0.0f;
        const float d2 = (on && cl[k] + 2 < creal) ? v[k].z - mean : 0.0f;
        const float d3 = (on && cl[k] + 3 < creal) ? v[k].w - mean : 0.0f;
        sq += d0 * d0; sq += d1 * d1; sq += d2 * d2; sq += d3 * d3;
    }
    const float rstd = 1.0f / sqrtf(gnp_block_sum(sq, red) * inv_cnt + 1e-5f);
    if (p.stats != nullptr && tid == 0) {
        float* st = p.stats + ((long)b * 8 + g) * 2;
        st[0] = mean; st[1] = rstd;
    }
    const float* tptr = p.temb != nullptr
                            ? p.temb + (p.trow != nullptr ? (long)p.trow[b] * p.temb_stride : 0L) + g * p.cpg
                            : nullptr;
    const float* gptr = p.gamma + g * p.cpg;
    const float* bptr = p.beta + g * p.cpg;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        if (off[k] < 0) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);   // zero-padded rows stay zero
        if (row[k] < lr) {
            const float4 ga = *reinterpret_cast<const float4*>(gptr + cl[k]);
            const float4 be = *reinterpret_cast<const float4*>(bptr + cl[k]);
            o.x = mish_fast_f32((v[k].x - mean) * rstd * ga.x + be.x);
            o.y = mish_fast_f32((v[k].y - mean) * rstd * ga.y + be.y);
            o.z = mish_fast_f32((v[k].z - mean) * rstd * ga.z + be.z);
            o.w = mish_fast_f32((v[k].w - mean) * rstd * ga.w + be.w);
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tptr != nullptr) a = *reinterpret_cast<const float4*>(tptr + cl[k]);
            if (p.res != nullptr) {
                const float4 r = *reinterpret_cast<const float4*>(p.res + off[k]);
                a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
            }
            o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
        }
        *reinterpret_cast<float4*>(p.dst + off[k]) = o;
    }
}

}  // namespace dad
