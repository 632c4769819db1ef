// conv_halo8.hpp — the 5-tap stride-1 fp32 convs of 8-position layers at full-chip batches, without the products
// that read nothing but the zero halo.
//
// A "same" conv over 8 positions reads halo rows in 6 of its 40 (tap, position) products per sample.  conv_gemm_f32
// orders a wave's 32 MFMA columns as 4 samples x 8 positions, so every v_mfma_f32_32x32x2_f32 mixes halo and real
// rows and nothing can be left out.  Here the tile's 64 columns are position-pair-major (conv_shapes.hpp, halo8_*):
// four blocks of 16 columns, block q = positions {2q, 2q + 1} of the tile's eight samples, multiplied with
// v_mfma_f32_16x16x4_f32 (same FLOP rate, same exact fp32 arithmetic).  Of a wave tile's twenty (tap, block)
// products two read only halo rows — tap offset -2 on block 0, +2 on block 3 — and each of the two wave tiles along
// N owns one of them: 10 % of the K-loop MFMAs, the same share for every wave (the split-K waves split channels).
// Which product is skipped is a compile-time property of (tap index, block): wave tile 1 walks its blocks and the
// taps mirrored (halo8_block / halo8_tap), which costs a wave-uniform sign on two address strides and no branch.
//
// Everything else is conv_gemm_f32's <BM, 64, SK, 32, 5, 1, RAGGED = false, ..., RES> form: the LDS stage (one row
// per position with halo rows, per-sample slot shifts), the weight image, the rolling software pipeline, the
// exchange through LDS and the GroupNorm -> Mish -> time embedding -> residual tail with write-through stores; the
// riding 1x1 conv is the never-skipped centre tap.  What changes with the column order is each lane's fragment
// address and the accumulator -> exchange-tile row.
//
// Fragments: lane (i = lane & 15, kq = lane >> 4) holds channels 2kq, 2kq + 1 of an 8-channel unit, one ds_read_b64
// per block and unit (the same LDS bytes per MFMA cycle as the ds_read_b128 of the 32x32x2 loop).  A ds_read_b64 is
// served in two groups of 32 lanes and is conflict-free when the 32 eight-byte slots are distinct mod 32: weight
// rows are 18 slots apart (16 consecutive rows -> 16 distinct even slots, kq fills the odd ones); the activation
// rows need the per-sample shifts of find_xswz_pairs (host_plan.hpp), checked by tests/sanitize/halo8_check.cpp.
// (ds_read_b128 fragments — a 16-channel unit — cannot be made conflict-free here: its 16-lane groups mix two kq
// values, which forces all 16 rows of a block onto even 16-byte slots, and rows KC + 4 floats apart alternate.)
//
// Two forms of the same sum: conv_halo8_f32 stages the weights in LDS (32 x 32 wave tiles share a fragment along N);
// conv_halo8w_f32, below it, gives a wave 16 output channels x all 64 columns and reads its weights straight into the
// MFMA's registers.  Bit-identical; the planner picks per (tile, ride) (host_plan.hpp choose_halo8, halo8w_faster).
//
// Not built: L = 16 (a 64-row tile holds 4 samples: no 16-column block is all halo), L = 4, the
// split-f16, direct-B, ragged, padded and windowed forms, the training forward, grid split-K.
#pragma once
#include "conv_gemm.hpp"

namespace dad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int BM, int SK, bool RES>
__global__ __launch_bounds__(64 * (BM / 32) * 2 * SK) void conv_halo8_f32(const ConvParams p) {
    constexpr int BN = 64, KC = 32, TAPS = 5, PAD = TAPS / 2, L = 8, LSH = 3;
    constexpr int TMW = BM / 32, TNW = BN / 32, WT = TMW * TNW, NT = 64 * WT * SK;
    constexpr int WTAPS = TAPS + (RES ? 1 : 0);
    constexpr int KP = KC + 4;
    constexpr int KU = 8;                        // channels per unit: 2 k-steps of v_mfma_f32_16x16x4_f32
    constexpr int G = KC / KU, GW = G / SK;
    constexpr int KG = 16, NSUB = KC / KG;
    constexpr int SPT = BN / L, SEG = L + 2 * PAD, XROWS = SPT * SEG;
    constexpr int XF = XROWS * KP + kXSwzPad;
    constexpr int STAGE = XF + WTAPS * BM * KP;  // floats per stage: [X rows][W rows]
    constexpr int STAGE4 = STAGE / 4, STAGE2 = STAGE / 2;
    static_assert(BN == 2 * 32 && G % SK == 0 && GW >= 1 && STAGE % 4 == 0, "tile shape");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* const smem4 = reinterpret_cast<float4*>(smem);
    float2* const smem2 = reinterpret_cast<float2*>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wt = wave % WT;
    const int ks = wave / WT;                    // split-K slice of this wave
    const int tn = wt / TMW;
    const int tm = wt % TMW;
    const int i16 = lane & 15;
    const int kq = lane >> 4;

    int mt = blockIdx.y;
    int nt = blockIdx.z;
    if (p.xcd_gn > 0) {                          // XCD-aware tile order, as conv_gemm_f32
        const int wg = blockIdx.y, c = wg & 7, j = wg >> 3;
        const int im = c / p.xcd_gn, in = c - im * p.xcd_gn;
        mt = (im << p.xcd_mts) + (j & ((1 << p.xcd_mts) - 1));
        nt = in * p.xcd_ntn + (j >> p.xcd_mts);
    }
    const int s0 = nt * SPT;                     // first sample of this tile
    const int m0 = mt * BM;                      // first output channel of this tile
    const int M = p.M;
    const int nvalid = min(SPT, p.B - s0);

    // A operand (activations): lane's (sample, position) of wave-tile block nb -> LDS row of tap index 0
    const int asmp = halo8_sample(i16);
    const int koff = ks * (GW * KU) + 2 * kq;    // this wave's channels of a chunk, this lane's pair of a unit
    const int tap_first = halo8_tap(tn, 0);      // wave-uniform: conv tap of tap index t = tap_first + t * tap_dir
    const int tap_dir = tn ? -1 : 1;
    int afrag2[2], bfrag2[2];                    // float2 units
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
        afrag2[nb] = ((asmp * SEG + halo8_pos(i16, halo8_block(tn, nb))) * KP + (int)((p.xswz >> (4 * asmp)) & 15) * 4 + koff) >> 1;
    // B operand (weights): lane's output channel of M block mb
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) bfrag2[mb] = (XF + (tm * 32 + mb * 16 + i16) * KP + koff) >> 1;

    // two accumulation chains (one per k-step of a unit) for each of the 2 x 2 blocks of 16 x 16
    f32x4 acc[2][2][2];                          // [k-step][N block][M block]
    f32x4 accr[2][2][2];                         // RES: the riding 1x1 conv
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int r = 0; r < 4; ++r) { acc[s][nb][mb][r] = 0.0f; accr[s][nb][mb][r] = 0.0f; }

    const int nchunks = (p.cin0 + p.cin1) / KC;  // whole chunks (host-checked), no grid split-K

    // ---- staging: global -> registers (prefetch) -> LDS, as conv_gemm_f32 (RAGGED = false) -------------------
    constexpr int W_F4 = WTAPS * BM * KC / 4;
    constexpr int W_PER_T = (W_F4 + NT - 1) / NT;
    constexpr int KQ = KC / 4;                   // float4 per row
    constexpr int X_PER_T = (BN * KQ + NT - 1) / NT;
    static_assert(X_PER_T * NT == BN * KQ, "every thread stages the same number of X items");
    float4 wreg[W_PER_T];
    float4 xreg[X_PER_T];
    int w_goff[W_PER_T], w_loff[W_PER_T];
    int x_grow[X_PER_T], x_q4[X_PER_T], x_loff[X_PER_T];
    constexpr int GQ = KG / 4;
#pragma unroll
    for (int i = 0; i < W_PER_T; ++i) {
        const int e = tid + i * NT;
        const int row = e / KQ;                  // tap*BM + m
        const int q = e - row * KQ;
        const int tap = row / BM;
        const int mm = row - tap * BM;
        const int sub = q / GQ;
        w_goff[i] = ((sub * p.wtaps + tap) * M + m0 + mm) * KG + (q - sub * GQ) * 4;
        w_loff[i] = (XF + row * KP + q * 4) >> 2;
    }
#pragma unroll
    for (int i = 0; i < X_PER_T; ++i) {
        const int e = tid + i * NT;
        const int row = e / KQ;                  // s*L + l
        const int q = e - row * KQ;
        const int s = row >> LSH;
        const int l = row - (s << LSH);
        x_grow[i] = s < nvalid ? s0 * L + row : -1;
        x_q4[i] = q * 4;
        x_loff[i] = ((s * SEG + PAD + l) * KP + q * 4 + (int)((p.xswz >> (4 * s)) & 15) * 4) >> 2;
    }
    const long w_chunk_stride = (long)NSUB * p.wtaps * M * KG;
    constexpr int NLD = W_PER_T + X_PER_T;
    auto item_store = [&](int k, int stage) {
        const int base4 = stage * STAGE4;
        if (k < W_PER_T) {
            if (W_F4 % NT == 0 || tid + k * NT < W_F4) smem4[base4 + w_loff[k]] = wreg[k];
        } else {
            const int i = k - W_PER_T;
            float4 v = xreg[i];
            if (x_grow[i] < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);   // no such sample
            smem4[base4 + x_loff[i]] = v;
        }
    };
    auto item_load = [&](int k, int chunk) {
        if (k < W_PER_T) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (W_F4 % NT == 0 || tid + k * NT < W_F4)
                v = *reinterpret_cast<const float4*>(p.w + chunk * w_chunk_stride + w_goff[k]);
            wreg[k] = v;
        } else {
            const int i = k - W_PER_T;
            const int c0 = chunk * KC;
            // whole chunk inside one source: one pointer per chunk, unconditional load (rows that do not exist read
            // row 0 and are zeroed at the store)
            const bool second = c0 >= p.cin0;
            const float* xsrc = second ? p.src1 : p.src0;
            const int cs = second ? p.cin1 : p.cin0;
            const int cb = second ? c0 - p.cin0 : c0;
            xreg[i] = *reinterpret_cast<const float4*>(xsrc + (long)max(x_grow[i], 0) * cs + cb + x_q4[i]);
        }
    };

    // ---- MFMA operand fragments: unit u = (tap index, 8-channel group of this wave) ---------------------------
    constexpr int UW = WTAPS * GW;
    auto frag_a = [&](int stage, int u, int nb) -> float2 {
        const int wtap = u / GW, gw = u - wtap * GW;
        const int tap = (RES && wtap == TAPS) ? PAD : tap_first + wtap * tap_dir;   // the 1x1 ride reads the centre rows
        return smem2[stage * STAGE2 + afrag2[nb] + tap * (KP / 2) + gw * (KU / 2)];
    };
    auto frag_b = [&](int stage, int u, int mb) -> float2 {
        const int wtap = u / GW, gw = u - wtap * GW;
        const int tap = (RES && wtap == TAPS) ? TAPS : tap_first + wtap * tap_dir;
        return smem2[stage * STAGE2 + bfrag2[mb] + tap * (BM * KP / 2) + gw * (KU / 2)];
    };

#pragma unroll
    for (int k = 0; k < NLD; ++k) item_load(k, 0);

    // ---- epilogue ownership (decided up front so its global loads can fly under the K loop), as conv_gemm_f32 --
    constexpr int ES = BM + 4;
    constexpr int ECOPY = BN * ES;
    constexpr int F4PL = (BN * BM / 4) / NT;
    static_assert(F4PL >= 1 && (BN * BM / 4) % NT == 0 && (F4PL & (F4PL - 1)) == 0, "epilogue mapping");
    const bool has_gn = p.gamma != nullptr;
    const int cpg = has_gn ? p.cpg : BM;
    const int cq = cpg >> 2;
    const int cnt4 = has_gn ? (L * cq) : (BN * cq);
    const int lpp = cnt4 >> (F4PL == 1 ? 0 : F4PL == 2 ? 1 : F4PL == 4 ? 2 : 3);
    const int lpp_sh = 31 - __clz(lpp);
    const int cq_sh = 31 - __clz(cq);
    const int gpt_sh = 31 - __clz(BM) - (31 - __clz(cpg));
    const int pr = tid >> lpp_sh;
    const int lp = tid & (lpp - 1);
    const int ps = has_gn ? pr >> gpt_sh : 0;
    const int pg = has_gn ? pr & ((1 << gpt_sh) - 1) : 0;
    int erow[F4PL], ecol[F4PL];
    int eoff[F4PL];
    float4 bias4[F4PL], gam4[F4PL], bet4[F4PL], temb4[F4PL], res4[F4PL];
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        const int j = lp + k * lpp;
        const int r = j >> cq_sh;
        erow[k] = ps * L + r;
        ecol[k] = pg * cpg + (j & (cq - 1)) * 4;
        const int s = erow[k] >> LSH;
        eoff[k] = ((s0 + s) * L + (erow[k] & (L - 1))) * M + m0 + ecol[k];
        if (s >= nvalid) eoff[k] = -1;
    }
    // every parameter load is unconditional: an absent operand reads the bias row and is cancelled by a select
    const float* const gptr = has_gn ? p.gamma : p.bias;
    const float* const bptr = has_gn ? p.beta : p.bias;
    const float* const tptr = p.temb != nullptr ? p.temb : p.bias;
    const bool has_res = p.res != nullptr;
    const bool has_temb = p.temb != nullptr;
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        const int em = m0 + ecol[k];
        long toff = 0;
        if (p.trow != nullptr)                   // per-row timesteps
            toff = (long)p.trow[min(s0 + (erow[k] >> LSH), p.B - 1)] * p.temb_stride;
        bias4[k] = ldg4(p.bias + em);
        gam4[k] = ldg4(gptr + em);
        bet4[k] = ldg4(bptr + em);
        temb4[k] = ldg4(tptr + toff + em);
        res4[k] = ldg4(has_res ? p.res + max(eoff[k], 0) : p.bias + em);
    }
    // zero the halo rows of both X stages once (real rows are rewritten in full by every chunk's staging)
    {
        constexpr int KP4 = KP / 4;
        constexpr int nz = SPT * (2 * PAD) * KP4;
        for (int i = tid; i < nz; i += NT) {
            const int hr = i / KP4, c4 = i - hr * KP4;
            const int s = hr / (2 * PAD), j = hr - s * (2 * PAD);
            const int row = s * SEG + (j < PAD ? j : L + j);
            const int at = row * KP + c4 * 4 + (int)((p.xswz >> (4 * s)) & 15) * 4;
            smem4[at >> 2] = make_float4(0.f, 0.f, 0.f, 0.f);
            smem4[STAGE4 + (at >> 2)] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
#pragma unroll
    for (int k = 0; k < NLD; ++k) item_store(k, 0);
    if (1 < nchunks) {
#pragma unroll
        for (int k = 0; k < NLD; ++k) item_load(k, 1);
    }
    __syncthreads();

    // ---- main loop: conv_gemm_f32's rolling pipeline; a unit is 8 channels = 2 k-steps x (2 x 2 blocks) of
    // v_mfma_f32_16x16x4_f32, minus block 0 at tap index 0 (all halo) ----------------------------------------------
    float2 a0 = make_float2(0.f, 0.f), a1 = frag_a(0, 0, 1), b0 = frag_b(0, 0, 0), b1 = frag_b(0, 0, 1);
#define DAD8_ROLL(STORE, LOAD)                                                                   \
    _Pragma("unroll") for (int k = 0; k < NLD; ++k) {                                            \
        if ((k * UW) / NLD != u) continue;                                                       \
        if (STORE) item_store(k, cur ^ 1);                                                       \
        if (LOAD) item_load(k, ch + 2);                                                          \
    }
#define DAD8_READ(ST, U)                                                                         \
    if ((U) / GW != 0) na0 = frag_a(ST, U, 0);   /* (tap index 0, block 0): never multiplied */  \
    na1 = frag_a(ST, U, 1);                                                                      \
    nb0 = frag_b(ST, U, 0);                                                                      \
    nb1 = frag_b(ST, U, 1);
#define DAD8_STEP(ACC, S, AX0, AX1, BX0, BX1, SKIP0)                                             \
    if (!(SKIP0)) {                                                                              \
        ACC[S][0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(AX0, BX0, ACC[S][0][0], 0, 0, 0);    \
        ACC[S][0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(AX0, BX1, ACC[S][0][1], 0, 0, 0);    \
    }                                                                                            \
    ACC[S][1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(AX1, BX0, ACC[S][1][0], 0, 0, 0);        \
    ACC[S][1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(AX1, BX1, ACC[S][1][1], 0, 0, 0);
#define DAD8_MFMA()                                                                              \
    if (RES && u / GW == TAPS) {                                                                 \
        DAD8_STEP(accr, 0, a0.x, a1.x, b0.x, b1.x, false)                                        \
        DAD8_STEP(accr, 1, a0.y, a1.y, b0.y, b1.y, false)                                        \
    } else {                                                                                     \
        DAD8_STEP(acc, 0, a0.x, a1.x, b0.x, b1.x, u / GW == 0)                                   \
        DAD8_STEP(acc, 1, a0.y, a1.y, b0.y, b1.y, u / GW == 0)                                   \
    }
    // STORE: chunk ch+1 exists (its operands go to the other stage); LOAD: chunk ch+2 exists
#define DAD8_CHUNK(STORE, LOAD)                                                                  \
    {                                                                                            \
        const int cur = ch & 1;                                                                  \
        _Pragma("unroll") for (int u = 0; u < UW; ++u) {                                         \
            float2 na0 = a0, na1 = a1, nb0 = b0, nb1 = b1;                                       \
            DAD8_ROLL(STORE, LOAD)                                                               \
            if (u + 1 < UW) {                                                                    \
                DAD8_READ(cur, u + 1)                                                            \
            } else {                                                                             \
                __syncthreads();                                                                 \
                if (STORE) { DAD8_READ(cur ^ 1, 0) }                                             \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            DAD8_MFMA()                                                                          \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;                                              \
        }                                                                                        \
    }
    int ch = 0;
    for (; ch + 2 < nchunks; ++ch) DAD8_CHUNK(true, true)
    if (ch + 1 < nchunks) { DAD8_CHUNK(true, false) ++ch; }
    if (ch < nchunks) DAD8_CHUNK(false, false)
#undef DAD8_CHUNK
#undef DAD8_MFMA
#undef DAD8_STEP
#undef DAD8_READ
#undef DAD8_ROLL
    __syncthreads();                             // all MFMAs retired before the stage memory is reused

    // ---- epilogue: conv_gemm_f32's, with this kernel's accumulator -> tile row map -----------------------------
    float* E = smem;                             // [SK][BN][ES]
    float* red = smem + SK * ECOPY;              // [2][waves] cross-wave partials
    // (a macro, not a lambda: accumulators captured by reference would be parked in scratch)
#define DAD8_DROP(A)                                                                             \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb)                                             \
    _Pragma("unroll") for (int mb = 0; mb < 2; ++mb)                                             \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                              \
        const int i = 4 * kq + r;                /* MFMA row of accumulator register r */        \
        const int row = halo8_sample(i) * L + halo8_pos(i, halo8_block(tn, nb));                 \
        const int col = tm * 32 + mb * 16 + i16;                                                 \
        E[ks * ECOPY + row * ES + col] = A[0][nb][mb][r] + A[1][nb][mb][r];                      \
    }
    DAD8_DROP(acc)
    __syncthreads();

    float y[F4PL][4];
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        const float* q = E + erow[k] * ES + ecol[k];
        float4 v = *reinterpret_cast<const float4*>(q);
#pragma unroll
        for (int c = 1; c < SK; ++c) {
            const float4 u = *reinterpret_cast<const float4*>(q + c * ECOPY);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        y[k][0] = v.x; y[k][1] = v.y; y[k][2] = v.z; y[k][3] = v.w;
    }

    if constexpr (RES) {
        // the riding 1x1 conv: same exchange, same ownership, bias, store
        __syncthreads();                         // every thread has read its main-tile values
        DAD8_DROP(accr)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < F4PL; ++k) {
            const float* q = E + erow[k] * ES + ecol[k];
            float4 v = *reinterpret_cast<const float4*>(q);
#pragma unroll
            for (int c = 1; c < SK; ++c) {
                const float4 u = *reinterpret_cast<const float4*>(q + c * ECOPY);
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            const float4 rb = ldg4(p.rbias + m0 + ecol[k]);
            if (eoff[k] >= 0)
                store_f4_sc1(p.rdst + eoff[k], make_float4(v.x + rb.x, v.y + rb.y, v.z + rb.z, v.w + rb.w));
        }
    }
#undef DAD8_DROP
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        y[k][0] += bias4[k].x; y[k][1] += bias4[k].y; y[k][2] += bias4[k].z; y[k][3] += bias4[k].w;
    }

    if (has_gn) {
        const float inv_cnt = 1.0f / (float)(cnt4 * 4);
        const int width = lpp < 64 ? lpp : 64;
        const int wpp = lpp >> 6;                // waves per pair when a pair spans waves
        auto pair_sum = [&](float v, int slot) -> float {
            if (width >= 2) v += dpp_f32<0xB1>(v);
            if (width >= 4) v += dpp_f32<0x4E>(v);
            if (width >= 8) v += dpp_f32<0x141>(v);
            if (width >= 16) v += dpp_f32<0x140>(v);
            if (width >= 32) v = rows_sum(v, width, lane);
            if (wpp > 1) {                       // block-uniform branch
                if (lane == 0) red[slot * 16 + wave] = v;
                __syncthreads();
                const int w0 = (wave / wpp) * wpp;
                v = 0.0f;
                for (int w = 0; w < wpp; ++w) v += red[slot * 16 + w0 + w];
            }
            return v;
        };
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < F4PL; ++k) sum += (y[k][0] + y[k][1]) + (y[k][2] + y[k][3]);
        const float mean = pair_sum(sum, 0) * inv_cnt;
        float sq = 0.0f;
#pragma unroll
        for (int k = 0; k < F4PL; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float d = y[k][c] - mean; sq += d * d; }
        const float rstd = 1.0f / sqrtf(pair_sum(sq, 1) * inv_cnt + 1e-5f);
#pragma unroll
        for (int k = 0; k < F4PL; ++k) {
            y[k][0] = mish_fast_f32((y[k][0] - mean) * rstd * gam4[k].x + bet4[k].x);
            y[k][1] = mish_fast_f32((y[k][1] - mean) * rstd * gam4[k].y + bet4[k].y);
            y[k][2] = mish_fast_f32((y[k][2] - mean) * rstd * gam4[k].z + bet4[k].z);
            y[k][3] = mish_fast_f32((y[k][3] - mean) * rstd * gam4[k].w + bet4[k].w);
        }
    }
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        if (eoff[k] < 0) continue;
        const float4 t4 = has_temb ? temb4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 r4 = has_res ? res4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        store_f4_sc1(p.dst + eoff[k], make_float4(y[k][0] + (t4.x + r4.x), y[k][1] + (t4.y + r4.y),
                                                  y[k][2] + (t4.z + r4.z), y[k][3] + (t4.w + r4.w)));
    }
}

// ---- the register-weight form -------------------------------------------------------------------------------------
// The same tile, arithmetic and summation order with the block cut into wave tiles the other way: a wave owns one
// M block of 16 output channels and all four column blocks (BM / 16 M blocks x SK K slices = 8 waves on both tiles).
// A weight fragment is then used by exactly one wave, so it needs no LDS: each lane reads its float2 (output channel
// tm * 16 + i16, channels 2kq, 2kq + 1 of an 8-channel unit) from the packed image straight into the register the
// MFMA takes it from — 16 rows x 32 bytes per load instruction, the other half of every 64-byte row by the wave's
// other unit or its K-slice neighbour — and every weight byte is still fetched once per block.  The stage holds the
// X rows alone (halo8w_lds_floats: the exchange tile of the epilogue is now the larger need).
//
// Summation order: blocks 0 and 1 walk the taps upwards and blocks 2 and 3 downwards, as wave tiles 0 and 1 of
// conv_halo8_f32 do, here as a compile-time choice per block: unit (tap index t, group) multiplies blocks 0, 1 with
// tap t and blocks 2, 3 with tap 4 - t, so both all-halo products — (tap 0, block 0), (tap 4, block 3) — fall on tap
// index 0 of every wave.  The k-step chains, the K slices and the exchange are the same: every output element adds
// the same products in the same order, and the result is bit-identical to conv_halo8_f32's.
//
// A tap's weights are used at two units of a chunk (t and 4 - t), so a wave holds its whole chunk of fragments
// (WTAPS x GW float2) and loads the next chunk's into a second set while it multiplies: unconditional loads in the
// first half of the units, the X row's store and reload after them, one register copy per fragment at the chunk's end
// (v_mov in the shadow of the last MFMAs) — the oldest outstanding load is always the one waited for.
template <int BM, int SK, bool RES>
__global__ __launch_bounds__(64 * (BM / 16) * SK) void conv_halo8w_f32(const ConvParams p) {
    constexpr int BN = 64, KC = 32, TAPS = 5, PAD = TAPS / 2, L = 8, LSH = 3;
    constexpr int TMW = BM / 16, NT = 64 * TMW * SK;
    constexpr int WTAPS = TAPS + (RES ? 1 : 0);
    constexpr int KP = KC + 4;
    constexpr int KU = 8;                        // channels per unit: 2 k-steps of v_mfma_f32_16x16x4_f32
    constexpr int G = KC / KU, GW = G / SK;
    constexpr int KG = 16, NSUB = KC / KG;
    constexpr int SPT = BN / L, SEG = L + 2 * PAD, XROWS = SPT * SEG;
    constexpr int STAGE = XROWS * KP + kXSwzPad; // floats per stage: the X rows
    constexpr int STAGE4 = STAGE / 4, STAGE2 = STAGE / 2;
    static_assert(BM % 16 == 0 && G % SK == 0 && GW >= 1 && STAGE % 4 == 0 && NT == 512, "tile shape");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* const smem4 = reinterpret_cast<float4*>(smem);
    float2* const smem2 = reinterpret_cast<float2*>(smem);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tm = wave % TMW;                   // M block (16 output channels) of this wave
    const int ks = wave / TMW;                   // split-K slice of this wave
    const int i16 = lane & 15;
    const int kq = lane >> 4;

    int mt = blockIdx.y;
    int nt = blockIdx.z;
    if (p.xcd_gn > 0) {                          // XCD-aware tile order, as conv_gemm_f32
        const int wg = blockIdx.y, c = wg & 7, j = wg >> 3;
        const int im = c / p.xcd_gn, in = c - im * p.xcd_gn;
        mt = (im << p.xcd_mts) + (j & ((1 << p.xcd_mts) - 1));
        nt = in * p.xcd_ntn + (j >> p.xcd_mts);
    }
    const int s0 = nt * SPT;                     // first sample of this tile
    const int m0 = mt * BM;                      // first output channel of this tile
    const int M = p.M;
    const int nvalid = min(SPT, p.B - s0);

    // A operand (activations): the lane's (sample, position) of block 0 at tap 0; block q is 2q rows further
    const int asmp = halo8_sample(i16);
    const int koff = ks * (GW * KU) + 2 * kq;    // this wave's channels of a chunk, this lane's pair of a unit
    const int afrag2 = ((asmp * SEG + halo8_pos(i16, 0)) * KP + (int)((p.xswz >> (4 * asmp)) & 15) * 4 + koff) >> 1;
    // B operand (weights): the lane's float2 of (slot 0, group 0) in the image [ci / 16][slot][M][ci % 16]
    const float* const wsrc = p.w + ((long)(m0 + tm * 16 + i16) * KG + 2 * kq);
    const long w_chunk_stride = (long)NSUB * p.wtaps * M * KG;
    auto w_load = [&](int k, int chunk) -> float2 {
        const int slot = k / GW, gw = k - slot * GW;
        const int c8 = (ks * GW + gw) * KU;      // wave-uniform: first channel of the unit within the chunk
        return *reinterpret_cast<const float2*>(wsrc + chunk * w_chunk_stride + (long)(((c8 / KG) * p.wtaps + slot) * M) * KG + c8 % KG);
    };

    // two accumulation chains (one per k-step of a unit) for each of the four blocks of 16 x 16
    f32x4 acc[2][4];                             // [k-step][block]
    f32x4 accr[2][4];                            // RES: the riding 1x1 conv
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) { acc[s][q][r] = 0.0f; accr[s][q][r] = 0.0f; }

    const int nchunks = (p.cin0 + p.cin1) / KC;  // whole chunks (host-checked), no grid split-K

    // ---- X staging: global -> registers (prefetch) -> LDS, as conv_halo8_f32 -------------------------------------
    constexpr int NW = WTAPS * GW;               // weight fragments of this wave per chunk
    constexpr int KQ = KC / 4;                   // float4 per row
    constexpr int X_PER_T = BN * KQ / NT;
    static_assert(X_PER_T == 1, "every thread stages one X item");
    float2 wcur[NW], wnxt[NW];
    float4 xreg;
    int x_grow, x_q4, x_loff;
    {
        const int row = tid / KQ;                // s*L + l
        const int q = tid - row * KQ;
        const int s = row >> LSH;
        const int l = row - (s << LSH);
        x_grow = s < nvalid ? s0 * L + row : -1;
        x_q4 = q * 4;
        x_loff = ((s * SEG + PAD + l) * KP + q * 4 + (int)((p.xswz >> (4 * s)) & 15) * 4) >> 2;
    }
    auto x_store = [&](int stage) {
        float4 v = xreg;
        if (x_grow < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);          // no such sample
        smem4[stage * STAGE4 + x_loff] = v;
    };
    auto x_load = [&](int chunk) {
        const int c0 = chunk * KC;
        // whole chunk inside one source: one pointer per chunk, unconditional load (rows that do not exist read
        // row 0 and are zeroed at the store)
        const bool second = c0 >= p.cin0;
        const float* xsrc = second ? p.src1 : p.src0;
        const int cs = second ? p.cin1 : p.cin0;
        const int cb = second ? c0 - p.cin0 : c0;
        xreg = *reinterpret_cast<const float4*>(xsrc + (long)max(x_grow, 0) * cs + cb + x_q4);
    };

    // ---- MFMA operand fragments: unit u = (tap index, 8-channel group of this wave) ---------------------------
    constexpr int UW = WTAPS * GW;
    auto frag_a = [&](int stage, int u, int q) -> float2 {
        const int wtap = u / GW, gw = u - wtap * GW;
        const int tap = (RES && wtap == TAPS) ? PAD : (q < 2 ? wtap : TAPS - 1 - wtap);   // the 1x1 ride reads the centre rows
        return smem2[stage * STAGE2 + afrag2 + q * KP + tap * (KP / 2) + gw * (KU / 2)];
    };

    x_load(0);
#pragma unroll
    for (int k = 0; k < NW; ++k) wcur[k] = wnxt[k] = w_load(k, 0);

    // ---- epilogue ownership (decided up front so its global loads can fly under the K loop), as conv_gemm_f32 --
    constexpr int ES = BM + 4;
    constexpr int ECOPY = BN * ES;
    constexpr int F4PL = (BN * BM / 4) / NT;
    static_assert(F4PL >= 1 && (BN * BM / 4) % NT == 0 && (F4PL & (F4PL - 1)) == 0, "epilogue mapping");
    const bool has_gn = p.gamma != nullptr;
    const int cpg = has_gn ? p.cpg : BM;
    const int cq = cpg >> 2;
    const int cnt4 = has_gn ? (L * cq) : (BN * cq);
    const int lpp = cnt4 >> (F4PL == 1 ? 0 : F4PL == 2 ? 1 : F4PL == 4 ? 2 : 3);
    const int lpp_sh = 31 - __clz(lpp);
    const int cq_sh = 31 - __clz(cq);
    const int gpt_sh = 31 - __clz(BM) - (31 - __clz(cpg));
    const int pr = tid >> lpp_sh;
    const int lp = tid & (lpp - 1);
    const int ps = has_gn ? pr >> gpt_sh : 0;
    const int pg = has_gn ? pr & ((1 << gpt_sh) - 1) : 0;
    int erow[F4PL], ecol[F4PL];
    int eoff[F4PL];
    float4 bias4[F4PL], gam4[F4PL], bet4[F4PL], temb4[F4PL], res4[F4PL];
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        const int j = lp + k * lpp;
        const int r = j >> cq_sh;
        erow[k] = ps * L + r;
        ecol[k] = pg * cpg + (j & (cq - 1)) * 4;
        const int s = erow[k] >> LSH;
        eoff[k] = ((s0 + s) * L + (erow[k] & (L - 1))) * M + m0 + ecol[k];
        if (s >= nvalid) eoff[k] = -1;
    }
    // every parameter load is unconditional: an absent operand reads the bias row and is cancelled by a select
    const float* const gptr = has_gn ? p.gamma : p.bias;
    const float* const bptr = has_gn ? p.beta : p.bias;
    const float* const tptr = p.temb != nullptr ? p.temb : p.bias;
    const bool has_res = p.res != nullptr;
    const bool has_temb = p.temb != nullptr;
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        const int em = m0 + ecol[k];
        long toff = 0;
        if (p.trow != nullptr)                   // per-row timesteps
            toff = (long)p.trow[min(s0 + (erow[k] >> LSH), p.B - 1)] * p.temb_stride;
        bias4[k] = ldg4(p.bias + em);
        gam4[k] = ldg4(gptr + em);
        bet4[k] = ldg4(bptr + em);
        temb4[k] = ldg4(tptr + toff + em);
        res4[k] = ldg4(has_res ? p.res + max(eoff[k], 0) : p.bias + em);
    }
    // zero the halo rows of both X stages once (real rows are rewritten in full by every chunk's staging)
    {
        constexpr int KP4 = KP / 4;
        constexpr int nz = SPT * (2 * PAD) * KP4;
        for (int i = tid; i < nz; i += NT) {
            const int hr = i / KP4, c4 = i - hr * KP4;
            const int s = hr / (2 * PAD), j = hr - s * (2 * PAD);
            const int row = s * SEG + (j < PAD ? j : L + j);
            const int at = row * KP + c4 * 4 + (int)((p.xswz >> (4 * s)) & 15) * 4;
            smem4[at >> 2] = make_float4(0.f, 0.f, 0.f, 0.f);
            smem4[STAGE4 + (at >> 2)] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    x_store(0);
    if (1 < nchunks) x_load(1);
    __syncthreads();

    // ---- main loop: a unit is 8 channels = 2 k-steps x 4 blocks of v_mfma_f32_16x16x4_f32, minus blocks 0 and 3 at
    // tap index 0 (all halo).  During chunk ch the weights of ch + 1 arrive in wnxt, X of ch + 1 goes to the other
    // stage and X of ch + 2 into xreg ------------------------------------------------------------------------------
    constexpr int XU = (NW + 1) / 2;             // the unit after the last weight load
    static_assert(XU < UW, "the X item rolls inside the chunk");
    float2 a[4];
    a[0] = a[3] = make_float2(0.f, 0.f);
    a[1] = frag_a(0, 0, 1);
    a[2] = frag_a(0, 0, 2);
#define DAD8W_ROLL(STORE, LOAD)                                                                  \
    _Pragma("unroll") for (int k = 0; k < NW; ++k) {                                             \
        if (k / 2 != u) continue;                                                                \
        if (STORE) wnxt[k] = w_load(k, ch + 1);                                                  \
    }                                                                                            \
    if (u == XU) {                                                                               \
        if (STORE) x_store(cur ^ 1);                                                             \
        if (LOAD) x_load(ch + 2);                                                                \
    }
#define DAD8W_READ(ST, U)                                                                        \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                \
        if ((U) / GW != 0 || (q != 0 && q != 3)) na[q] = frag_a(ST, U, q);   /* tap index 0, blocks 0 and 3: never multiplied */
#define DAD8W_STEP(ACC, S, C, B01, B23, SKIP)                                                    \
    if (!(SKIP)) ACC[S][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0].C, B01.C, ACC[S][0], 0, 0, 0); \
    ACC[S][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1].C, B01.C, ACC[S][1], 0, 0, 0);         \
    ACC[S][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2].C, B23.C, ACC[S][2], 0, 0, 0);         \
    if (!(SKIP)) ACC[S][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3].C, B23.C, ACC[S][3], 0, 0, 0);
#define DAD8W_MFMA()                                                                             \
    if (RES && u / GW == TAPS) {                                                                 \
        const float2 b = wcur[u];                                                                \
        DAD8W_STEP(accr, 0, x, b, b, false)                                                      \
        DAD8W_STEP(accr, 1, y, b, b, false)                                                      \
    } else {                                                                                     \
        const float2 b01 = wcur[u], b23 = wcur[(TAPS - 1 - u / GW) * GW + u % GW];               \
        DAD8W_STEP(acc, 0, x, b01, b23, u / GW == 0)                                             \
        DAD8W_STEP(acc, 1, y, b01, b23, u / GW == 0)                                             \
    }
    // STORE: chunk ch+1 exists (its X rows go to the other stage, its weights to wnxt); LOAD: chunk ch+2 exists
#define DAD8W_CHUNK(STORE, LOAD)                                                                 \
    {                                                                                            \
        const int cur = ch & 1;                                                                  \
        _Pragma("unroll") for (int u = 0; u < UW; ++u) {                                         \
            float2 na[4] = {a[0], a[1], a[2], a[3]};                                             \
            DAD8W_ROLL(STORE, LOAD)                                                              \
            if (u + 1 < UW) {                                                                    \
                DAD8W_READ(cur, u + 1)                                                           \
            } else {                                                                             \
                __syncthreads();                                                                 \
                if (STORE) { DAD8W_READ(cur ^ 1, 0) }                                            \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            DAD8W_MFMA()                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) a[q] = na[q];                          \
        }                                                                                        \
        if (STORE) {                                                                             \
            _Pragma("unroll") for (int k = 0; k < NW; ++k) wcur[k] = wnxt[k];                    \
        }                                                                                        \
    }
    int ch = 0;
    for (; ch + 2 < nchunks; ++ch) DAD8W_CHUNK(true, true)
    if (ch + 1 < nchunks) { DAD8W_CHUNK(true, false) ++ch; }
    if (ch < nchunks) DAD8W_CHUNK(false, false)
#undef DAD8W_CHUNK
#undef DAD8W_MFMA
#undef DAD8W_STEP
#undef DAD8W_READ
#undef DAD8W_ROLL
    __syncthreads();                             // all MFMAs retired before the stage memory is reused

    // ---- epilogue: conv_halo8_f32's, with this kernel's accumulator -> tile row map ------------------------------
    float* E = smem;                             // [SK][BN][ES]
    float* red = smem + SK * ECOPY;              // [2][waves] cross-wave partials
#define DAD8W_DROP(A)                                                                            \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                              \
        const int i = 4 * kq + r;                /* MFMA row of accumulator register r */        \
        const int row = halo8_sample(i) * L + halo8_pos(i, q);                                   \
        const int col = tm * 16 + i16;                                                           \
        E[ks * ECOPY + row * ES + col] = A[0][q][r] + A[1][q][r];                                \
    }
    DAD8W_DROP(acc)
    __syncthreads();

    float y[F4PL][4];
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        const float* q = E + erow[k] * ES + ecol[k];
        float4 v = *reinterpret_cast<const float4*>(q);
#pragma unroll
        for (int c = 1; c < SK; ++c) {
            const float4 u = *reinterpret_cast<const float4*>(q + c * ECOPY);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
        }
        y[k][0] = v.x; y[k][1] = v.y; y[k][2] = v.z; y[k][3] = v.w;
    }

    if constexpr (RES) {
        // the riding 1x1 conv: same exchange, same ownership, bias, store
        __syncthreads();                         // every thread has read its main-tile values
        DAD8W_DROP(accr)
        __syncthreads();
#pragma unroll
        for (int k = 0; k < F4PL; ++k) {
            const float* q = E + erow[k] * ES + ecol[k];
            float4 v = *reinterpret_cast<const float4*>(q);
#pragma unroll
            for (int c = 1; c < SK; ++c) {
                const float4 u = *reinterpret_cast<const float4*>(q + c * ECOPY);
                v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
            }
            const float4 rb = ldg4(p.rbias + m0 + ecol[k]);
            if (eoff[k] >= 0)
                store_f4_sc1(p.rdst + eoff[k], make_float4(v.x + rb.x, v.y + rb.y, v.z + rb.z, v.w + rb.w));
        }
    }
#undef DAD8W_DROP
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        y[k][0] += bias4[k].x; y[k][1] += bias4[k].y; y[k][2] += bias4[k].z; y[k][3] += bias4[k].w;
    }

    if (has_gn) {
        const float inv_cnt = 1.0f / (float)(cnt4 * 4);
        const int width = lpp < 64 ? lpp : 64;
        const int wpp = lpp >> 6;                // waves per pair when a pair spans waves
        auto pair_sum = [&](float v, int slot) -> float {
            if (width >= 2) v += dpp_f32<0xB1>(v);
            if (width >= 4) v += dpp_f32<0x4E>(v);
            if (width >= 8) v += dpp_f32<0x141>(v);
            if (width >= 16) v += dpp_f32<0x140>(v);
            if (width >= 32) v = rows_sum(v, width, lane);
            if (wpp > 1) {                       // block-uniform branch
                if (lane == 0) red[slot * 16 + wave] = v;
                __syncthreads();
                const int w0 = (wave / wpp) * wpp;
                v = 0.0f;
                for (int w = 0; w < wpp; ++w) v += red[slot * 16 + w0 + w];
            }
            return v;
        };
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < F4PL; ++k) sum += (y[k][0] + y[k][1]) + (y[k][2] + y[k][3]);
        const float mean = pair_sum(sum, 0) * inv_cnt;
        float sq = 0.0f;
#pragma unroll
        for (int k = 0; k < F4PL; ++k)
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float d = y[k][c] - mean; sq += d * d; }
        const float rstd = 1.0f / sqrtf(pair_sum(sq, 1) * inv_cnt + 1e-5f);
#pragma unroll
        for (int k = 0; k < F4PL; ++k) {
            y[k][0] = mish_fast_f32((y[k][0] - mean) * rstd * gam4[k].x + bet4[k].x);
            y[k][1] = mish_fast_f32((y[k][1] - mean) * rstd * gam4[k].y + bet4[k].y);
            y[k][2] = mish_fast_f32((y[k][2] - mean) * rstd * gam4[k].z + bet4[k].z);
            y[k][3] = mish_fast_f32((y[k][3] - mean) * rstd * gam4[k].w + bet4[k].w);
        }
    }
#pragma unroll
    for (int k = 0; k < F4PL; ++k) {
        if (eoff[k] < 0) continue;
        const float4 t4 = has_temb ? temb4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 r4 = has_res ? res4[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        store_f4_sc1(p.dst + eoff[k], make_float4(y[k][0] + (t4.x + r4.x), y[k][1] + (t4.y + r4.y),
                                                  y[k][2] + (t4.z + r4.z), y[k][3] + (t4.w + r4.w)));
    }
}

}  // namespace dad
