// conv_seam.hpp — the seam between two denoise steps of the sampling loop as one launch: final_conv[1] and the
// posterior update of step t (pointwise.hpp, final_posterior_kernel) and the first conv of the evaluation at t - 1
// (downs.0.0.blocks.0: transition_dim -> dim, 5 taps, with the block's riding 1x1 residual conv).
//
// The posterior of row (b, l) needs that row's `dim` activations only, the first conv of sample b needs sample b's
// new x only: a workgroup that owns 32 rows — 32 / H whole samples — and ALL output channels does both without any
// hand-off between workgroups.  x is updated in place as before (each element read and written by one thread of the
// grid); the new values also go straight into the conv's X stage in LDS, so the conv's activation operand never
// comes from HBM, and only the 8-channel units that hold real channels are multiplied.
//
// Same bits as the two launches it replaces (tests/test_hip_seam.py):
//   * the posterior is pointwise.hpp's final_dots<1> and final_posterior_kernel's update (posterior_finish), per output;
//   * the conv keeps conv_gemm_f32's summation structure for the tile the planner gave the first conv (T0: tile 0,
//     32 x 64 SK4 KC32 — every 8-channel unit is its own split-K copy, the copies are added in unit order; else
//     tile 1, 64 x 64 SK2 KC32 — both units run through one set of chains, tap-major): chain i = channels {i, 4 + i}
//     of a unit, taps ascending, four chains summed pairwise, the ride on two chains of its own reading the centre
//     rows.  Every product left out is an exact +0 onto a sum that is never -0;
//   * the GroupNorm statistics are conv_gemm_f32's reduction trees for that tile: a thread here owns two float4 of
//     one (sample, group) pair — the two float4 of one thread of tile 1 (F4PL = 2), or those of two neighbouring
//     threads of tile 0 (F4PL = 1), whose first butterfly level then happens in registers.
//
// LDS (conv_shapes.hpp seam_lds_floats): [32][dim + 4] activation tile (the exchange tile afterwards) | [td][dim]
// final_conv[1] weights | bias | X stage: 32 / H samples x (H + 4) rows of SEAM_KP floats with the per-sample slot
// shifts of find_xswz | [32][dim + 4] exchange tile of the ride.  The conv's weights go global -> registers (every
// fragment is used by one wave).  Three barriers: staged -> posterior -> conv -> epilogue.  No spin-waits, no
// cross-block hand-offs.
//
// final_act may be the very buffer the conv writes (the activation allocator hands final_conv[0] the first free
// level-0 buffer, which is the first conv's): both are [B * H][dim] row-major, a workgroup reads its 32 rows of it
// in full before the first barrier and stores the same 32 rows after the last one, and touches no other row.
#pragma once
#include "pointwise.hpp"

namespace dad {

struct SeamParams {
    FinalParams f;      // the posterior update of step t (x, noise, schedule scalars, draw / seed of t)
    ConvParams c;       // the first conv of the evaluation at t - 1 (temb: row t - 1 of the table)
    int32_t units;      // 8-channel units that hold real channels: 1 (td <= 8) or 2
    int32_t hshift;     // log2(horizon)
};

// Posterior update of output j of position n = (b, l) (diffusion.py:159-223, policies.py:84-110): the `finish` lambda
// of final_posterior_kernel (pointwise.hpp), statement for statement, as a function — acc is the dot product of
// final_conv[1], xv the element's x_t, bl the staged biases, zpre the injected noise loaded ahead (read only when
// p.noise is set).  Returns true when x was written, xn the value.  (The lambda stays where it is: calling this
// function from that kernel instead permutes its scalar registers, and its instruction stream is kept as it was;
// tests/test_hip_seam.py holds the two to the same bits on every option.)
// Roundings as that kernel compiles: hipcc forms its two-term sums from v_pk_mul_f32 products — c_recip * x -
// c_recipm1 * out and coef1 * x0 + coef2 * x are two products and an add, no FMA — and contracts guide and noise
// (v_fmac_f32).  Here, with one output per thread at dim 128, it contracted the former as well (1 ulp of x on a fifth
// of the elements): they run with contraction off, the latter are written as fmaf.  The guide's shift of x0 (the DDIM
// form of guidance, FinalParams.guide_x0) is an explicit fmaf in all three copies: one rounding, whatever is contracted.
__device__ __forceinline__ bool posterior_finish(const FinalParams& p, const float* bl, long n, int td, int b, int l, int j,
                                                 float acc, float xv, float zpre, float& xn) {
    const long idx = n * td + j;
    const float out = acc + bl[j];
    if (p.eps_out != nullptr) p.eps_out[idx] = out;
    if (p.x_out_disabled && p.mean_out == nullptr) return false;
    float x0 = out, mean;
    {
#pragma clang fp contract(off)
        if (p.predict_epsilon) x0 = p.c_recip * xv - p.c_recipm1 * out;
        if (p.guide != nullptr) x0 = fmaf(p.guide_x0, p.guide[idx], x0);
        if (p.clip_denoised) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
        mean = p.coef1 * x0 + p.coef2 * xv;
    }
    if (p.guide != nullptr) mean = fmaf(p.guide_scale, p.guide[idx], mean);
    if (p.mean_out != nullptr) p.mean_out[idx] = mean;
    if (p.x_out_disabled) return false;
    const float z = (p.noise != nullptr)
                        ? zpre
                        : philox_normal(p.elem_offset + (uint64_t)idx, p.draw,
                                        p.seed_dev != nullptr ? (uint64_t)*p.seed_dev : p.seed);
    xn = fmaf(p.sigma, z, mean);
    if (l == 0 && p.cond0 != nullptr) xn = p.cond0[(p.cond_per_row ? (long)b * td : 0) + j];
    p.x[idx] = xn;
    return true;
}

// store_f4_sc1 (conv_gemm.hpp) followed by wait states.  An asm store is invisible to hipcc: nothing keeps it from
// re-using the data registers in the very next VALU instruction, and the hazard recognizer does not see a store in the
// asm statement.  Behind the ride's store this kernel has address arithmetic left to do, and at full-chip batches
// the first data register was overwritten (an integer in every fourth channel of a few rows of rdst) before the
// store had read it.
__device__ __forceinline__ void seam_store_f4_sc1(float* p, const float4 v) {
    typedef float __attribute__((ext_vector_type(4))) f4;
    const f4 x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 7" ::"v"(p), "v"(x) : "memory");
}

template <int DIM, bool T0>
__global__ __launch_bounds__(4 * DIM) void conv_seam_f32(const SeamParams q) {
    constexpr int NT = seam_threads(DIM), TMW = DIM / 32, ES = DIM + 4, KP = SEAM_KP, TAPS = 5, PAD = TAPS / 2;
    constexpr int JG = NT / 32;                  // threads per position in the posterior phase
    constexpr int JB = 16 / JG;                  // outputs per thread: td <= 16
    constexpr int DQ = DIM / 4;
    static_assert(DIM == 32 || DIM == 64 || DIM == 128, "dim");
    static_assert(T0 || DIM >= 64, "tile 1 needs 64 output channels");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* const smem4 = reinterpret_cast<float4*>(smem);
    const FinalParams& p = q.f;
    const ConvParams& c = q.c;
    const int td = p.td, H = p.H, hsh = q.hshift;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31;
    const int h = lane >> 5;
    const int SPT = 32 >> hsh, SEG = H + 2 * PAD;
    const int XF = seam_xf(H);
    float* const tile = smem;                    // [32][ES]; the conv's exchange tile after the posterior
    float* const wl = tile + 32 * ES;            // [td][DIM]
    float* const bl = wl + td * DIM;             // [td] (+ pad to 4)
    float* const xs = bl + ((td + 3) & ~3);      // X stage
    float* const ER = xs + XF;                   // [32][ES] the ride's exchange tile
    const int xs4 = (int)(xs - smem) >> 2;       // (every offset above is a multiple of 4 floats)
    const long N = (long)p.B * H;
    const long n0 = (long)blockIdx.x * 32;
    const int s0 = (int)blockIdx.x * SPT;        // first sample of this tile
    const int nvalid = min(SPT, p.B - s0);
    const int M = c.M;

    // ---- 1. every load first ----------------------------------------------------------------------------------
    // (unconditional, clamped addresses: a load under a condition costs a drained s_waitcnt — conv_gemm.hpp)
    float4 areg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + i * NT;
        const int row = e / DQ, qd = e - row * DQ;
        areg[i] = ldg4(p.act + min(n0 + row, N - 1) * DIM + qd * 4);
    }
    const float4 wreg = ldg4(p.w + (long)min(tid, td * DQ - 1) * 4);
    const float breg = p.bias[min(tid, td - 1)];
    const int col = tid & 31;
    const int jg = tid >> 5;
    const long n = n0 + col;
    const long nc = min(n, N - 1);
    const float* const zsrc = p.noise != nullptr ? p.noise : p.x;     // absent: any readable tensor of the shape
    float xv[JB], zv[JB];
#pragma unroll
    for (int k = 0; k < JB; ++k) {
        const long at = nc * td + min(jg + k * JG, td - 1);
        xv[k] = p.x[at];
        zv[k] = zsrc[at];
    }
    // the conv's weight fragments, straight from the packed image [granule 0][tap slot][M][16]: waves [0, TMW) own the
    // five taps of their 32 channels, waves [TMW, 2 TMW) the ride (tap slot 5)
    const bool rider = wave >= TMW;
    const int tm = rider ? wave - TMW : wave;
    float4 wf[TAPS][2];
    {
        const float* const base = c.w + (long)(tm * 32 + l32) * 16 + 4 * h;
#pragma unroll
        for (int t = 0; t < TAPS; ++t)
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int slot = rider ? TAPS : t;                      // (the ride re-reads one slot: five L1 hits)
                wf[t][g] = ldg4(base + (long)slot * M * 16 + g * 8);
            }
    }
    // epilogue ownership: two float4 of one (sample, group) pair per thread, in conv_gemm_f32's order for the tile
    constexpr int CPG = DIM / 8, CQ = CPG / 4;   // channels / float4 per row of a pair
    constexpr int CQ_SH = CQ == 1 ? 0 : CQ == 2 ? 1 : 2;
    const int cnt4 = H * CQ;                     // float4 per pair
    const int lpp = T0 ? cnt4 : cnt4 >> 1;       // that kernel's lanes per pair
    const int lpp_sh = 31 - __clz(lpp);
    int erow[2], ecol[2], eoff[2];
    float4 bias4[2], gam4[2], bet4[2], temb4[2], rb4[2];
    const float* const tptr = c.temb != nullptr ? c.temb : c.bias;
    const bool has_temb = c.temb != nullptr;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int vt = T0 ? 2 * tid + k : tid;   // that kernel's thread
        const int pr = vt >> lpp_sh, lp = vt & (lpp - 1);
        const int ps = pr >> 3, pg = pr & 7;
        const int j = T0 ? lp : lp + k * lpp;
        erow[k] = ps * H + (j >> CQ_SH);
        ecol[k] = pg * CPG + (j & (CQ - 1)) * 4;
        const int s = erow[k] >> hsh;
        eoff[k] = ((s0 + s) * H + (erow[k] & (H - 1))) * M + ecol[k];
        if (s >= nvalid) eoff[k] = -1;
        bias4[k] = ldg4(c.bias + ecol[k]);
        gam4[k] = ldg4(c.gamma + ecol[k]);
        bet4[k] = ldg4(c.beta + ecol[k]);
        temb4[k] = ldg4(tptr + ecol[k]);
        rb4[k] = ldg4(c.rbias + ecol[k]);
    }

    // ---- 2. stage: zeros over the whole X stage (halo rows, channels >= td, samples beyond the batch), the
    //         activation tile, final_conv[1] -------------------------------------------------------------------
    for (int i = tid; i < (XF >> 2); i += NT) smem4[xs4 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + i * NT;
        const int row = e / DQ, qd = e - row * DQ;
        float4 v = areg[i];
        if (n0 + row >= N) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(tile + row * ES + qd * 4) = v;
    }
    if (tid < td * DQ) *reinterpret_cast<float4*>(wl + tid * 4) = wreg;
    if (tid < td) bl[tid] = breg;
    __syncthreads();

    // ---- 3. posterior of this block's 32 rows: x in place, and into the X stage ------------------------------
    if (n < N) {
        const int s = col >> hsh, l = col & (H - 1);
        const int b = s0 + s;
        float* const xrow = xs + (s * SEG + PAD + l) * KP + (int)((c.xswz >> (4 * s)) & 15) * 4;
#pragma unroll
        for (int k = 0; k < JB; ++k) {
            const int j = jg + k * JG;
            if (j >= td) continue;
            float acc;
            final_dots<1>(wl + j * DIM, tile + col * ES, DIM, 0, &acc);
            float xn;
            if (posterior_finish(p, bl, n, td, b, l, j, acc, xv[k], zv[k], xn)) xrow[j] = xn;
        }
    }
    __syncthreads();

    // ---- 4. conv: one K chunk, the units with real channels only ---------------------------------------------
    {
        const int arow4 = xs4 + ((((l32 >> hsh) * SEG + (l32 & (H - 1))) * KP + 4 * h) >> 2) + (int)((c.xswz >> (4 * (l32 >> hsh))) & 15);
        auto frag_a = [&](int tap, int g) -> float4 { return smem4[arow4 + tap * (KP / 4) + g * 2]; };
        const int units = q.units;
        f32x16 tot;
        if (!rider) {
            f32x16 a1, a2, a3, a4;
#pragma unroll
            for (int r = 0; r < 16; ++r) { a1[r] = 0.0f; a2[r] = 0.0f; a3[r] = 0.0f; a4[r] = 0.0f; tot[r] = 0.0f; }
#define DAD_SEAM_MAIN(T, G)                                                                      \
    {                                                                                            \
        const float4 a = frag_a(T, G), w = wf[T][G];                                             \
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, a1, 0, 0, 0);                        \
        a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, a2, 0, 0, 0);                        \
        a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, a3, 0, 0, 0);                        \
        a4 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, a4, 0, 0, 0);                        \
    }
            if constexpr (T0) {
                // tile 0: unit g is split-K copy g; the copies meet in unit order
#pragma unroll
                for (int t = 0; t < TAPS; ++t) DAD_SEAM_MAIN(t, 0)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[r] = (a1[r] + a2[r]) + (a3[r] + a4[r]);
                if (units > 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { a1[r] = 0.0f; a2[r] = 0.0f; a3[r] = 0.0f; a4[r] = 0.0f; }
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) DAD_SEAM_MAIN(t, 1)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot[r] += (a1[r] + a2[r]) + (a3[r] + a4[r]);
                }
            } else {
                // tile 1: one wave owns both units, tap-major
                if (units > 1) {
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) { DAD_SEAM_MAIN(t, 0) DAD_SEAM_MAIN(t, 1) }
                } else {
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) DAD_SEAM_MAIN(t, 0)
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[r] = (a1[r] + a2[r]) + (a3[r] + a4[r]);
            }
#undef DAD_SEAM_MAIN
        } else {
            f32x16 r1, r2;
#pragma unroll
            for (int r = 0; r < 16; ++r) { r1[r] = 0.0f; r2[r] = 0.0f; tot[r] = 0.0f; }
#define DAD_SEAM_RIDE(G)                                                                         \
    {                                                                                            \
        const float4 a = frag_a(PAD, G), w = wf[0][G];                                           \
        r1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, r1, 0, 0, 0);                        \
        r2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, r2, 0, 0, 0);                        \
        r1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, r1, 0, 0, 0);                        \
        r2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, r2, 0, 0, 0);                        \
    }
            DAD_SEAM_RIDE(0)
            if constexpr (T0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[r] = r1[r] + r2[r];
                if (units > 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { r1[r] = 0.0f; r2[r] = 0.0f; }
                    DAD_SEAM_RIDE(1)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tot[r] += r1[r] + r2[r];
                }
            } else {
                if (units > 1) DAD_SEAM_RIDE(1)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[r] = r1[r] + r2[r];
            }
#undef DAD_SEAM_RIDE
        }
        // (the activation tile was last read in front of the barrier above: it is the exchange tile now)
        float* const E = rider ? ER : tile;
#pragma unroll
        for (int r = 0; r < 16; ++r) E[((r & 3) + 8 * (r >> 2) + 4 * h) * ES + tm * 32 + l32] = tot[r];
    }
    __syncthreads();

    // ---- 5. epilogue: conv_gemm_f32's — ride: bias, store; conv: bias -> GroupNorm -> Mish -> + time embedding ----
    float y[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float4 r = *reinterpret_cast<const float4*>(ER + erow[k] * ES + ecol[k]);
        if (eoff[k] >= 0)
            seam_store_f4_sc1(c.rdst + eoff[k], make_float4(r.x + rb4[k].x, r.y + rb4[k].y, r.z + rb4[k].z, r.w + rb4[k].w));
        const float4 v = *reinterpret_cast<const float4*>(tile + erow[k] * ES + ecol[k]);
        y[k][0] = v.x; y[k][1] = v.y; y[k][2] = v.z; y[k][3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        y[k][0] += bias4[k].x; y[k][1] += bias4[k].y; y[k][2] += bias4[k].z; y[k][3] += bias4[k].w;
    }
    {
        const float inv_cnt = 1.0f / (float)(cnt4 * 4);
        const int vwidth = lpp < 64 ? lpp : 64;          // lanes of that kernel's in-wave reduction
        const int width = T0 ? vwidth >> 1 : vwidth;     // ... and ours: T0 did the first level in registers
        auto pair_sum = [&](float v) -> float {
            if (width >= 2) v += dpp_f32<0xB1>(v);
            if (width >= 4) v += dpp_f32<0x4E>(v);
            if (width >= 8) v += dpp_f32<0x141>(v);
            if (width >= 16) v += dpp_f32<0x140>(v);
            if (width >= 32) v = rows_sum(v, width, lane);
            if (T0 && lpp > 64) {
                // a pair of 128 lanes there spans two waves, added in wave order from 0; here they are the two halves
                // of this wave
                const int iv = __builtin_bit_cast(int, v);
                const float w0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
                const float w1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
                v = 0.0f;
                v += w0;
                v += w1;
            }
            return v;
        };
        float sum;
        if constexpr (T0) {
            float sa = 0.0f, sb = 0.0f;
            sa += (y[0][0] + y[0][1]) + (y[0][2] + y[0][3]);
            sb += (y[1][0] + y[1][1]) + (y[1][2] + y[1][3]);
            sum = sa + sb;
        } else {
            sum = 0.0f;
#pragma unroll
            for (int k = 0; k < 2; ++k) sum += (y[k][0] + y[k][1]) + (y[k][2] + y[k][3]);
        }
        const float mean = pair_sum(sum) * inv_cnt;
        // conv_gemm_f32's `sq += d * d` compiles, on both tiles, to the squares followed by a serial sum — no FMA (the
        // squares are formed in pairs, v_pk_mul_f32).  Left to the compiler the two four-element chains of T0 become
        // v_pk_fma_f32 chains here, one rounding fewer per term: contraction is switched off for this sum instead.
        float sq;
        {
#pragma clang fp contract(off)
            float dd[2][4];
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) { const float d = y[k][cc] - mean; dd[k][cc] = d * d; }
            const float qa = ((dd[0][0] + dd[0][1]) + dd[0][2]) + dd[0][3];
            if constexpr (T0) {
                const float qb = ((dd[1][0] + dd[1][1]) + dd[1][2]) + dd[1][3];
                sq = qa + qb;
            } else {
                sq = (((qa + dd[1][0]) + dd[1][1]) + dd[1][2]) + dd[1][3];
            }
        }
        const float rstd = 1.0f / sqrtf(pair_sum(sq) * inv_cnt + 1e-5f);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            y[k][0] = mish_fast_f32((y[k][0] - mean) * rstd * gam4[k].x + bet4[k].x);
            y[k][1] = mish_fast_f32((y[k][1] - mean) * rstd * gam4[k].y + bet4[k].y);
            y[k][2] = mish_fast_f32((y[k][2] - mean) * rstd * gam4[k].z + bet4[k].z);
            y[k][3] = mish_fast_f32((y[k][3] - mean) * rstd * gam4[k].w + bet4[k].w);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (eoff[k] < 0) continue;
        const float4 t4 = has_temb ? temb4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);      // (the first conv of a block has no residual operand)
        seam_store_f4_sc1(c.dst + eoff[k], make_float4(y[k][0] + (t4.x + r4.x), y[k][1] + (t4.y + r4.y),
                                                  y[k][2] + (t4.z + r4.z), y[k][3] + (t4.w + r4.w)));
    }
}

}  // namespace dad
