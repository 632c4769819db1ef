// optim_step.hpp — the optimiser step of dad_optim_step (include/dad.h): clip_grad_norm_, torch.optim.Adam and the
// EMA update of the reference's Trainer.train_step (utils/training.py:158-189) over a LIST of tensors in two
// launches.  Memory-bound: per element the update reads p, g, m, v, ema and writes p, m, v, ema (36 B), the
// square-sum pass reads g (4 B).
//
// Work split (csrc/host_plan.hpp: optim_plan): chunks of kOptimChunk elements numbered tensor by tensor, block b
// walks chunks [b * per_block, (b + 1) * per_block) in ascending order; it finds the tensor of its first chunk by
// bisection over first[] and steps to the next tensor as the chunk number passes first[t + 1].  A chunk starts at
// a multiple of 4 elements of its tensor, so a tensor whose pointers are 16-byte aligned (OptimDesc::vec) is
// accessed as float4 with a scalar tail; any other tensor one element at a time.
//
// Summation order of the squared norm: a thread adds its elements in chunk order into four lanes, the lanes and
// then the threads of a block are added by a fixed tree (optim_block_sum), the block's partial goes to
// partials[blockIdx.x]; every block of the update pass adds the partials with the same strided loop and tree.
// No atomics anywhere: the same plan gives the same bits.  The sums are kept in double (the pass is bound by its
// 4 B / element of traffic, not by the adds), so the clip coefficient carries one fp32 rounding instead of the
// summation error of 1e8 terms: it scales every gradient.
#pragma once
#include <hip/hip_runtime.h>

#include "host_plan.hpp"

namespace dad {

using dadhost::OptimGeom;

constexpr int OPT_THREADS = 256;

struct OptimDesc {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;
    int64_t numel;
    int32_t group;
    int32_t vec;      // every pointer above is 16-byte aligned (or null)
};
struct OptimGroups { dad_optim_group g[dadhost::kOptimMaxGroups]; };

// first[lo] <= c < first[lo + 1]
__device__ inline int optim_find_tensor(const int* first, int n, int c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Sum of `v` over the block in a fixed order, returned to every thread: a shuffle tree inside each wave of 64, then
// the four wave sums in wave order.  `red` is 4 doubles of LDS.
__device__ inline double optim_block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sqsum_kernel(const OptimDesc* __restrict__ descs,
                                                                  const int* __restrict__ first, int n, OptimGeom geom,
                                                                  double* __restrict__ partials) {
    __shared__ double red[4];
    int lo, hi;
    dadhost::optim_block_chunks(geom, (int)blockIdx.x, lo, hi);
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    int t = optim_find_tensor(first, n, lo);
    for (int c = lo; c < hi; ++c) {
        while (c >= first[t + 1]) ++t;
        const float* gbase = descs[t].g;
        if (!gbase) continue;                     // EMA-only tensor: no gradient
        int64_t e0;
        int32_t cnt;
        dadhost::optim_chunk_span(geom, c, first[t], descs[t].numel, e0, cnt);
        const float* g = gbase + e0;
        if (descs[t].vec) {
            const int n4 = cnt >> 2;
            const float4* g4 = reinterpret_cast<const float4*>(g);
            for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
                const float4 x = g4[i];
                a0 += (double)x.x * x.x; a1 += (double)x.y * x.y; a2 += (double)x.z * x.z; a3 += (double)x.w * x.w;
            }
            const int i = (n4 << 2) + (int)threadIdx.x;
            if (i < cnt) a0 += (double)g[i] * g[i];
        } else {
            for (int i = threadIdx.x; i < cnt; i += OPT_THREADS) a0 += (double)g[i] * g[i];
        }
    }
    const double s = optim_block_sum((a0 + a1) + (a2 + a3), red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// torch.optim.Adam on one element, in the operation order of its multi-tensor form (lerp, mul + addcmul,
// sqrt / bias correction + eps, addcdiv); `coef` is the clip coefficient.
__device__ inline void optim_adam(float& p, float g, float& m, float& v, float coef, const dad_optim_group& h) {
    g = coef * g;
    if (h.weight_decay != 0.f) {
        if (h.decoupled) p = p * (1.f - h.lr * h.weight_decay);
        else g = g + h.weight_decay * p;
    }
    m = m + (g - m) * h.one_minus_beta1;
    v = v * h.beta2;                              // mul_, then addcmul_: v + value * (g * g)
    v = v + h.one_minus_beta2 * (g * g);
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = p - h.step_size * (m / denom);
}

// ema.mul_(d).add_(p, alpha = 1 - d): the product is rounded on its own (mul_ stores it), then self + alpha * other
__device__ inline float optim_ema(float ema, float p, float decay) { return __fmul_rn(ema, decay) + (1.f - decay) * p; }

// npart > 0: `partials` holds that many partial square sums (the grid of optim_sqsum_kernel).  max_norm <= 0: no clip.
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const OptimDesc* __restrict__ descs,
                                                                   const int* __restrict__ first, int n, OptimGeom geom,
                                                                   const OptimGroups groups, const double* __restrict__ partials,
                                                                   int npart, float max_norm, float ema_decay,
                                                                   float* __restrict__ norm_out) {
    __shared__ double red[4];
    float coef = 1.f;
    if (npart > 0) {
        double s = 0.;
        for (int i = threadIdx.x; i < npart; i += OPT_THREADS) s += partials[i];
        // clip_grad_norm_'s expression, evaluated in double and rounded once: the coefficient scales every gradient, and
        // in fp32 its three roundings (norm, sum, quotient) show twice over in exp_avg_sq
        const double norm = sqrt(optim_block_sum(s, red));
        if (max_norm > 0.f) {
            const double c = (double)max_norm / (norm + 1e-6);
            coef = c > 1. ? 1.f : (float)c;       // (a NaN norm gives a NaN coefficient, as torch.clamp does)
        }
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
    }
    int lo, hi;
    dadhost::optim_block_chunks(geom, (int)blockIdx.x, lo, hi);
    int t = optim_find_tensor(first, n, lo);
    for (int c = lo; c < hi; ++c) {
        while (c >= first[t + 1]) ++t;
        const OptimDesc d = descs[t];
        const dad_optim_group& h = groups.g[d.group];
        int64_t e0;
        int32_t cnt;
        dadhost::optim_chunk_span(geom, c, first[t], d.numel, e0, cnt);
        float* const p = d.p + e0;
        float* const ema = d.ema ? d.ema + e0 : nullptr;
        if (!d.g) {                               // EMA only
            int i0 = 0;
            if (d.vec) {
                const int n4 = cnt >> 2;
                const float4* p4 = reinterpret_cast<const float4*>(p);
                float4* e4 = reinterpret_cast<float4*>(ema);
                for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
                    const float4 x = p4[i];
                    float4 e = e4[i];
                    e.x = optim_ema(e.x, x.x, ema_decay); e.y = optim_ema(e.y, x.y, ema_decay);
                    e.z = optim_ema(e.z, x.z, ema_decay); e.w = optim_ema(e.w, x.w, ema_decay);
                    e4[i] = e;
                }
                i0 = n4 << 2;
            }
            for (int i = i0 + (int)threadIdx.x; i < cnt; i += OPT_THREADS) ema[i] = optim_ema(ema[i], p[i], ema_decay);
            continue;
        }
        const float* const g = d.g + e0;
        float* const m = d.m + e0;
        float* const v = d.v + e0;
        int i0 = 0;
        if (d.vec) {
            const int n4 = cnt >> 2;
            float4* p4 = reinterpret_cast<float4*>(p);
            const float4* g4 = reinterpret_cast<const float4*>(g);
            float4* m4 = reinterpret_cast<float4*>(m);
            float4* v4 = reinterpret_cast<float4*>(v);
            float4* e4 = reinterpret_cast<float4*>(ema);
            for (int i = threadIdx.x; i < n4; i += OPT_THREADS) {
                float4 x = p4[i], mm = m4[i], vv = v4[i];
                const float4 gg = g4[i];
                optim_adam(x.x, gg.x, mm.x, vv.x, coef, h);
                optim_adam(x.y, gg.y, mm.y, vv.y, coef, h);
                optim_adam(x.z, gg.z, mm.z, vv.z, coef, h);
                optim_adam(x.w, gg.w, mm.w, vv.w, coef, h);
                p4[i] = x; m4[i] = mm; v4[i] = vv;
                if (ema) {
                    float4 e = e4[i];
                    e.x = optim_ema(e.x, x.x, ema_decay); e.y = optim_ema(e.y, x.y, ema_decay);
                    e.z = optim_ema(e.z, x.z, ema_decay); e.w = optim_ema(e.w, x.w, ema_decay);
                    e4[i] = e;
                }
            }
            i0 = n4 << 2;
        }
        for (int i = i0 + (int)threadIdx.x; i < cnt; i += OPT_THREADS) {
            float x = p[i], mm = m[i], vv = v[i];
            optim_adam(x, g[i], mm, vv, coef, h);
            p[i] = x; m[i] = mm; v[i] = vv;
            if (ema) ema[i] = optim_ema(ema[i], x, ema_decay);
        }
    }
}

}  // namespace dad
