// dad_lib.hip — host side of libdad_hip.so: model state, weight packing, launch plan and
// the C ABI declared in include/dad.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <mutex>
#include <set>
#include <tuple>
#include <utility>

#include "../../include/dad.h"
#include "host_plan.hpp"
#include "conv_gemm.hpp"
#include "conv_halo8.hpp"
#include "conv_gn_pass.hpp"
#include "pointwise.hpp"
#include "violation_grad.hpp"
#include "conv_seam.hpp"
#include "conv_cc.hpp"
#include "conv_ccw.hpp"
#include "train_bwd.hpp"
#include "train_objective.hpp"
#include "optim_step.hpp"
#include "guide_mlp.hpp"

using namespace dadhost;

namespace {

#ifdef DAD_STAMPS
unsigned long long* g_stamps = nullptr;
#endif

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(DAD_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                            \
    } while (0)

// Everything a captured loop freezes: pointers, sizes and the scalars baked into its launches.
struct GraphKey {
    const void* x; const void* noise; const void* cond; const void* ws;
    const void* P; const void* obs_mean; const void* obs_std; const void* act_mean; const void* act_std;
    const void* proj_scratch;
    const void* guide_ptrs[3 * DAD_GUIDE_MAX_LAYERS + 1];    // the guide's weight images, biases and gradient scratch
    int guide_shape[2 * DAD_GUIDE_MAX_LAYERS + 3];           //   its layers, widths and activation
    float guide_weight;
    int n_steps, batch, cond_per_row, state_dim, observation_dim, action_dim;
    int force_tile, flags;    // tile / split-K / fusion hooks change the captured launches
    uint64_t row_offset;
    uint64_t alpha_hash;      // projection strengths are baked into the captured launches
    uint64_t steps_hash;      //   and so are the coefficients of every step (the sampler)
    bool operator<(const GraphKey& o) const {
        return std::memcmp(this, &o, sizeof(GraphKey)) < 0;
    }
};

}  // namespace

struct dad_model : HostModel {
    bool finalized = false;
    int device = -1;                                           // device the parameters live on
    std::vector<float> sched[5];                               // host schedule scalars
    bool have_sched = false;
    std::vector<float> emb_override;                           // dad_model_load_time_embedding
    // device
    float* d_emb = nullptr;           // [T][dim]      SinusoidalPosEmb
    float* d_temb = nullptr;          // [T][time_dim] time_mlp output
    float* d_temb_table = nullptr;    // [T][temb_width] every block's Mish -> Linear
    float* d_final_w = nullptr;       // [td][dim]
    float* d_final_b = nullptr;
    uint64_t* d_rng = nullptr;
    unsigned* d_counters = nullptr;   // split-K arrival tickets (zero between launches)
    float* d_zero = nullptr;          // zeros: bias row of the data-gradient launches (training)
    std::map<std::string, float*> d_time;    // time-MLP tensors as uploaded (dad_model_refresh_weights re-derives the tables)
    std::vector<WeightEntry> weights;        // every device copy of a parameter (dad_model_refresh_weights rebuilds them)
    float* d_h1 = nullptr;            // [T][4 time_dim] scratch of the table builder
    std::vector<float> train_sched[2];         // dad_model_load_train_schedule: sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod
    float* d_train_sched = nullptr;   // [2][T] their device copy (made when the model is finalized, or at the load after it)
    float* d_recip_sched = nullptr;   // [2][T] device copy of sched[0], sched[1] (sqrt_recip / sqrt_recipm1_alphas_cumprod): made by the
    bool recip_sched_stale = true;    //   first dynamics-aware objective call behind a dad_model_load_schedule
    std::vector<void*> owned;         // every hipMalloc to free
    void* d_repack = nullptr;         // dad_model_refresh_weights: descriptor table of the last refresh (device)
    size_t repack_cap = 0;
    std::vector<char> repack_host;    //   and its host copy (re-uploaded only when it changes)
    bool tables_stale = false;        // time-MLP tensors changed since the per-timestep tables were built
    // All parameters, tables and flags live in ONE device allocation: a conv launch touches a
    // handful of pages instead of one page per tensor (cold address translations used to cost
    // ~1 us at the start of every kernel).
    char* arena = nullptr;
    size_t arena_cap = 0, arena_used = 0;
    // profiling
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    double prof_flops = 0;
    int64_t prof_launches = 0;
    // graphs
    std::map<GraphKey, hipGraphExec_t> graphs;
    hipStream_t cap_stream = nullptr;
};

namespace {

using dad::ConvParams;

int arena_alloc(dad_model* m, size_t bytes, void** out) {
    const size_t aligned = (bytes + 255) / 256 * 256;
    if (m->arena_used + aligned > m->arena_cap)
        return fail(DAD_E_STATE, "parameter arena exhausted (%zu + %zu > %zu)", m->arena_used, aligned,
                    m->arena_cap);
    *out = m->arena + m->arena_used;
    m->arena_used += aligned;
    return DAD_OK;
}

int upload(dad_model* m, const std::vector<float>& host, float** dev) {
    void* p = nullptr;
    const int rc = arena_alloc(m, std::max<size_t>(host.size(), 1) * sizeof(float), &p);
    if (rc != DAD_OK) return rc;
    HIP_TRY(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    *dev = (float*)p;
    return DAD_OK;
}

// The pointer through which the launches read the device copy of a weight-table entry.
float*& weight_ptr(dad_model* m, const WeightEntry& e) {
    switch (e.to) {
        case WT_W: return m->plan.convs[e.conv].d_w;
        case WT_BIAS: return m->plan.convs[e.conv].d_bias;
        case WT_RBIAS: return m->plan.convs[e.conv].d_rbias;
        case WT_GAMMA: return m->plan.convs[e.conv].d_gamma;
        case WT_BETA: return m->plan.convs[e.conv].d_beta;
        case WT_BWD_W: return m->bconvs[e.conv].op[e.sub].d_w;
        case WT_BFINAL_W: return m->bfinal.d_w;
        case WT_FINAL_W: return m->d_final_w;
        case WT_FINAL_B: return m->d_final_b;
        case WT_TIME: break;
    }
    return m->d_time[e.key];
}

void free_device(dad_model* m) {
    for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
    m->graphs.clear();
    for (void* p : m->owned) (void)hipFree(p);
    m->owned.clear();
    m->d_repack = nullptr; m->repack_cap = 0; m->repack_host.clear(); m->tables_stale = false;
    m->arena = nullptr;
    m->arena_cap = m->arena_used = 0;
    m->d_emb = m->d_temb = m->d_temb_table = nullptr;
    m->d_final_w = m->d_final_b = nullptr;
    m->d_rng = nullptr;
    m->d_counters = nullptr;
    m->d_zero = nullptr;
    m->d_train_sched = nullptr;
    m->weights.clear(); m->d_time.clear();
    for (Plan* plan : {&m->plan, &m->tplan})
        for (auto& op : plan->convs) op.d_w = op.d_bias = op.d_gamma = op.d_beta = op.d_rbias = nullptr;
    for (auto& b : m->bconvs) for (int k = 0; k < b.n; ++k) b.op[k].d_w = b.op[k].d_bias = nullptr;
    m->bfinal.d_w = m->bfinal.d_bias = nullptr;
}

// ---------------------------------------------------------------------- kernel registry
// Every instantiated kernel a launch looks up, of every family of kFamilies (host_plan.hpp).  Which ones exist is
// decided by the families' predicates and nowhere else: the table is filled by a compile-time walk over each
// family's whole domain, which instantiates kernel_of<family, key...> where family_kernel_exists holds.
//
// The instantiation a key names, per family (the key's ints as kFamilies orders them):
template <int CFG, int TAPS, int STRIDE, int F>
const void* gemm_kernel_of() {
    constexpr TileCfg T = kTiles[CFG];
    constexpr bool X3 = F & 1, BDIR = F & 2, RAGGED = F & 4, RES = F & 8, PADDED = F & 16, WIN = F & 32;
    return (const void*)dad::conv_gemm_f32<T.BM, T.BN, T.SK, tile_kc(CFG, TAPS, X3, BDIR), TAPS, STRIDE, RAGGED, X3, BDIR, RES, PADDED, WIN>;
}
template <int TAPS, int STRIDE, int RIDE, int BIG, int ROWS, int WIN>
const void* cc_kernel_of() { return (const void*)dad::conv_cc<TAPS, STRIDE, RIDE != 0, BIG != 0, ROWS, 6, WIN != 0>; }
template <int TAPS, int STRIDE, int RIDE, int RIDE_IN, int ROWS>
const void* ccw_kernel_of() { return (const void*)dad::conv_ccw<TAPS, STRIDE, RIDE != 0, RIDE_IN != 0, ROWS>; }
template <int CFG, int RIDE>
const void* halo8_kernel_of() {       // the block tile of kTiles[CFG]
    static_assert(kTiles[CFG].BN == 64 && kTiles[CFG].KC == 32, "conv_halo8_f32 has 64-position tiles and 32-channel K chunks");
    return (const void*)dad::conv_halo8_f32<kTiles[CFG].BM, kTiles[CFG].SK, RIDE != 0>;
}
template <int DIM, int TILE0>
const void* seam_kernel_of() { return (const void*)dad::conv_seam_f32<DIM, TILE0 != 0>; }
template <int TAPS, int TILE, int WIN>
const void* wgrad_kernel_of() {       // tiles 0..2: 64 x 64, 64 x 32, 32 x 32; tile 3: 32 x 32 with the general staging path
    return (const void*)dad::conv_wgrad<TAPS, TILE < 2 ? 2 : 1, TILE < 1 ? 2 : 1, TILE != 3, WIN != 0>;
}
template <int FAMILY, int... K>
const void* kernel_of() {
    if constexpr (FAMILY == FAM_GEMM) return gemm_kernel_of<K...>();
    else if constexpr (FAMILY == FAM_CC) return cc_kernel_of<K...>();
    else if constexpr (FAMILY == FAM_CCW) return ccw_kernel_of<K...>();
    else if constexpr (FAMILY == FAM_HALO8) return halo8_kernel_of<K...>();
    else if constexpr (FAMILY == FAM_SEAM) return seam_kernel_of<K...>();
    else { static_assert(FAMILY == FAM_WGRAD, "a family without a template"); return wgrad_kernel_of<K...>(); }
}

// One table for all families, sorted by the packed (family, key): a byte per int, the family on top.
struct KernelEntry { uint64_t key; const void* fn; };
using KernelTable = std::vector<KernelEntry>;
constexpr uint64_t kNoKey = ~0ull;            // what a key with an int outside 0..255 packs to: no entry has it
constexpr uint64_t pack_key(int family, const int* k, int n) {
    uint64_t key = (uint64_t)family;
    for (int i = 0; i < kMaxKeyInts; ++i) {
        const int v = i < n ? k[i] : 0;
        if (v < 0 || v > 255) return kNoKey;
        key = key << 8 | (uint64_t)v;
    }
    return key;
}
constexpr bool domains_pack() {               // every value of every domain fits its byte
    for (int f = 0; f < kNumFamilies; ++f)
        for (int a = 0; a < kFamilies[f].axes; ++a)
            for (int i = 0; i < kFamilies[f].axis[a].n; ++i)
                if (kFamilies[f].axis[a].at(i) < 0 || kFamilies[f].axis[a].at(i) > 255) return false;
    return kNumFamilies <= 256 && kMaxKeyInts <= 7;
}
static_assert(domains_pack(), "a kernel family's key does not pack into 64 bits");

// The walk: RegWalk<FAMILY, K...> has fixed the first sizeof...(K) ints of a key and runs over the next axis.  One fold
// per axis (a single fold over all combinations would exceed the compiler's nesting limit).
template <int FAMILY, int... K>
struct RegWalk {
    static constexpr int kFixed = sizeof...(K);
    static constexpr int kKey[kMaxKeyInts] = {K...};
    template <size_t... I>
    static void each(KernelTable& t, std::index_sequence<I...>) {
        (RegWalk<FAMILY, K..., kFamilies[FAMILY].axis[kFixed].at((int)I)>::run(t), ...);
    }
    static void run(KernelTable& t) {
        if constexpr (kFixed < kFamilies[FAMILY].axes) each(t, std::make_index_sequence<kFamilies[FAMILY].axis[kFixed].n>());
        else if constexpr (family_kernel_exists(FAMILY, kKey)) t.push_back({pack_key(FAMILY, kKey, kFixed), kernel_of<FAMILY, K...>()});
    }
};
template <size_t... FAMILY>
void reg_families(KernelTable& t, std::index_sequence<FAMILY...>) {
    (RegWalk<(int)FAMILY>::run(t), ...);
}
const KernelTable& kernel_table() {
    static const KernelTable table = [] {
        KernelTable t;
        reg_families(t, std::make_index_sequence<kNumFamilies>());
        std::sort(t.begin(), t.end(), [](const KernelEntry& a, const KernelEntry& b) { return a.key < b.key; });
        return t;
    }();
    return table;
}
// The kernel of a family's key (`n` ints), nullptr where the registry has none: every launch site refuses that.
const void* find_kernel(int family, const int* k, int n) {
    const uint64_t key = pack_key(family, k, n);
    const KernelTable& t = kernel_table();
    const auto it = std::lower_bound(t.begin(), t.end(), key, [](const KernelEntry& e, uint64_t v) { return e.key < v; });
    return it != t.end() && it->key == key ? it->fn : nullptr;
}
const void* find_kernel(int family, std::initializer_list<int> k) { return find_kernel(family, k.begin(), (int)k.size()); }

// The register-weight form of a FAM_HALO8 key (conv_halo8.hpp, conv_halo8w_f32): a second instantiation under the same
// (cfg, ride), generated from the family's predicate like the table — the registry's keys name the pair.
template <int CFG, int RIDE>
const void* halo8w_kernel_of() {
    if constexpr (halo8_kernel_exists(CFG, RIDE != 0)) return (const void*)dad::conv_halo8w_f32<kTiles[CFG].BM, kTiles[CFG].SK, RIDE != 0>;
    else return nullptr;
}
template <size_t... I>
const void* find_halo8w(int cfg, bool ride, std::index_sequence<I...>) {
    static const void* const fns[] = {halo8w_kernel_of<(int)I / 2, (int)I % 2>()...};
    return cfg >= 0 && cfg < kNumTiles ? fns[2 * cfg + (ride ? 1 : 0)] : nullptr;
}
const void* find_halo8w(int cfg, bool ride) { return find_halo8w(cfg, ride, std::make_index_sequence<2 * kNumTiles>()); }

// Every kernel may use up to the full 160 KiB of LDS; the dynamic-LDS limit is a per-device
// function attribute, raised once per device (not lazily per launch, so that nothing but launches
// happens under hipGraph capture).
int configure_kernels() {
    static std::mutex lock;
    static std::set<int> done;
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> hold(lock);
    if (done.count(dev)) return DAD_OK;
    std::vector<const void*> fns = {(const void*)dad::final_posterior_kernel, (const void*)dad::final_cc_kernel,
                                    (const void*)dad::project_kernel<4, 16>, (const void*)dad::project_kernel<1, 16>,
                                    (const void*)dad::violation_bwd_row_kernel, (const void*)dad::violation_fwd_gemm_kernel,
                                    (const void*)dad::violation_bwd_gemm_kernel,
                                    (const void*)dad::dynamics_violation_fwd_row_kernel<1, dad::PROJ_KP>,
                                    (const void*)dad::dynamics_violation_fwd_row_kernel<4, dad::PROJ_KP>,
                                    (const void*)dad::dynamics_violation_fwd_gemm_kernel, (const void*)dad::dynamics_violation_bwd_row_kernel,
                                    (const void*)dad::dynamics_violation_bwd_gemm_kernel,
                                    (const void*)dad::guide_mlp_kernel<dad::GUIDE_TANH>,
                                    (const void*)dad::guide_mlp_kernel<dad::GUIDE_RELU>,
                                    (const void*)dad::guide_mlp_kernel<dad::GUIDE_MISH>};
    for (const KernelEntry& e : kernel_table()) fns.push_back(e.fn);      // every family
    for (int cfg = 0; cfg < kNumTiles; ++cfg)
        for (int ride = 0; ride < 2; ++ride)
            if (const void* fn = find_halo8w(cfg, ride != 0)) fns.push_back(fn);
    for (const void* fn : fns)
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dad::kLdsBytes));
    done.insert(dev);
    return DAD_OK;
}

// Operands of one conv-GEMM launch as raw pointers (the forward plans name buffers; the backward walk
// passes gradient tensors).
struct ConvIO {
    const float* src0 = nullptr; const float* src1 = nullptr;
    float* dst = nullptr; const float* res = nullptr; float* rdst = nullptr;
    const float* temb = nullptr; const int32_t* trow = nullptr;
    float* pre = nullptr; float* stats = nullptr;      // training forward: pre-normalisation output, pair statistics
    float* slab = nullptr;                             // split-K scratch
};
int launch_conv(dad_model* m, const ConvOp& op, const LaunchGeom& g, int batch, const ConvIO& io, hipStream_t st);

// Launch `l` of the forward description `f`, on m->plan (sampling: buffers shared by lifetime) or m->tplan
// (training: every tensor kept, plus the pre-activation / statistics buffers of the GroupNorm'd convs).
// `temb_rows`: (B, temb_width) time projections of the training forward (indexed through trow), instead of the
// per-timestep table.
ConvIO conv_io(dad_model* m, const FwdPlan& f, const FwdLaunch& l, const float* xext, float* ws, int t,
               const int32_t* trow, const float* temb_rows) {
    const Plan& plan = f.train ? m->tplan : m->plan;
    const ConvOp& op = plan.convs[l.conv];
    const int batch = f.batch;
    auto buf = [&](int id) -> float* {
        return id >= 0 ? ws + plan.bufs[id].offset * (long)batch : nullptr;
    };
    ConvIO io;
    io.src0 = op.src0 == -2 ? xext : buf(op.src0);
    io.src1 = buf(op.src1);
    // shared timestep: row t of the table; per-row timesteps: row 0 + trow[b] * stride in the kernel
    if (op.temb_off >= 0)
        io.temb = temb_rows != nullptr ? temb_rows + op.temb_off
                                       : m->d_temb_table + (trow ? 0L : (long)t * m->plan.temb_width) + op.temb_off;
    // per-row timesteps only where there is a time embedding to index: the kernels' fallback operand
    // for an absent embedding is the bias row, which must not be offset by trow[b] * stride
    io.trow = io.temb != nullptr ? trow : nullptr;
    io.res = op.res == -2 ? xext : buf(op.res);       // identity residual of the trajectory itself (td == C)
    io.dst = buf(op.dst);
    io.rdst = buf(op.rdst);
    io.pre = buf(op.pre); io.stats = buf(op.stats);
    io.slab = ws + plan.floats_per_sample * (long)batch;     // scratch behind the activations
    return io;
}
int run_conv(dad_model* m, const FwdPlan& f, const FwdLaunch& l, const float* xext, float* ws, int t, hipStream_t st,
             const int32_t* trow, const float* temb_rows) {
    const Plan& plan = f.train ? m->tplan : m->plan;
    const ConvOp& op = plan.convs[l.conv];
    const int batch = f.batch;
    if (op.cat0 >= 0) {     // rows of [cat0 | cat1] side by side into the residual buffer
        auto buf = [&](int id) -> float* { return ws + plan.bufs[id].offset * (long)batch; };
        const long rows = (long)batch * op.Lout;
        const long n4 = rows * ((op.cat_c0 + op.cat_c1) / 4);
        hipLaunchKernelGGL(dad::concat_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                           buf(op.res), buf(op.cat0), buf(op.cat1), rows, op.cat_c0, op.cat_c1);
        HIP_TRY(hipGetLastError());
    }
    return launch_conv(m, op, l.g, batch, conv_io(m, f, l, xext, ws, t, trow, temb_rows), st);
}

// GroupNorm -> Mish -> + time embedding -> + residual of a windowed layer (conv_gn_pass.hpp), after its conv:
// gn_pass_kernel<npt>, npt planned with the launch (LaunchGeom::gn_npt)
int launch_gn_pass(dad_model* m, const ConvOp& op, int npt, int batch, const ConvIO& io, hipStream_t st) {
    dad::GnPassParams q{};
    q.src = io.pre != nullptr ? io.pre : io.dst;
    q.dst = io.dst;
    q.gamma = op.d_gamma; q.beta = op.d_beta;
    q.temb = io.temb; q.trow = io.trow; q.temb_stride = m->plan.temb_width;
    q.res = io.res; q.stats = io.stats;
    q.C = op.cout; q.L = op.Lout; q.cpg = op.cout / 8; q.lreal = op.lreal; q.cpg_real = op.gn_real;
    const dim3 grid(8, (unsigned)batch), block(dad::GNP_THREADS);
    static_assert(dad::kGnPassMaxNpt == 32, "one case per power of two up to kGnPassMaxNpt");
    switch (npt) {
        case 1: hipLaunchKernelGGL(dad::gn_pass_kernel<1>, grid, block, 0, st, q); break;
        case 2: hipLaunchKernelGGL(dad::gn_pass_kernel<2>, grid, block, 0, st, q); break;
        case 4: hipLaunchKernelGGL(dad::gn_pass_kernel<4>, grid, block, 0, st, q); break;
        case 8: hipLaunchKernelGGL(dad::gn_pass_kernel<8>, grid, block, 0, st, q); break;
        case 16: hipLaunchKernelGGL(dad::gn_pass_kernel<16>, grid, block, 0, st, q); break;
        default: hipLaunchKernelGGL(dad::gn_pass_kernel<32>, grid, block, 0, st, q);
    }
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

// `g`: the launch as plan_launch accepted it (plan_forward, train_scratch); nothing is decided here
ConvParams conv_params(dad_model* m, const ConvOp& op, const LaunchGeom& g, int batch, const ConvIO& io) {
    // windowed tiles of a GroupNorm'd layer: the conv stores conv + bias (into the pre-activation buffer when
    // the training forward keeps one), the pass over whole (sample, group) pairs finishes the block
    const bool gn_pass = g.gn_npt > 0;
    ConvParams p{};
    p.src0 = io.src0;
    p.src1 = io.src1;
    p.w = op.d_w; p.bias = op.d_bias; p.gamma = op.d_gamma; p.beta = op.d_beta;
    p.temb = io.temb;
    p.trow = io.trow; p.temb_stride = m->plan.temb_width;
    p.res = io.res;
    p.dst = io.dst;
    p.pre = io.pre; p.stats = io.stats;
    if (gn_pass) {
        p.gamma = p.beta = p.temb = p.res = nullptr;
        p.trow = nullptr;
        p.pre = nullptr; p.stats = nullptr;
        if (io.pre != nullptr) p.dst = io.pre;
    }
    p.cin0 = op.cin0; p.cin1 = op.cin1; p.cin_pad = op.cin_pad;
    p.M = op.M; p.cpg = op.norm.empty() ? 0 : op.cout / 8; p.cpg_real = op.gn_real;
    p.lreal = op.lreal; p.src_len = op.src_len;
    p.B = batch; p.Lin = op.Lin; p.Lout = op.Lout; p.lshift = ilog2(op.Lout);
    p.lshift_in = ilog2(op.Lin);
    p.interleave = op.kind == CONV_UP;
    p.ntiles_n = g.ntiles_n;
    p.xcd_gn = g.xcd_gn; p.xcd_mts = g.xcd_mts; p.xcd_ntn = g.xcd_ntn;
    p.kslices = g.split.kslices;
    p.chunks_per_slice = g.split.chunks_per_slice;
    p.slab = io.slab;
    p.counters = m->d_counters;
    p.c1 = op.c1; p.c2 = op.c2;
    p.xswz = g.xswz;
    p.wtaps = op.wtaps();
    p.rbias = g.fused ? op.d_rbias : nullptr;
    p.rdst = g.fused ? io.rdst : nullptr;
    return p;
}
int launch_conv(dad_model* m, const ConvOp& op, const LaunchGeom& g, int batch, const ConvIO& io, hipStream_t st) {
    const bool gn_pass = g.gn_npt > 0;
    ConvParams p = conv_params(m, op, g, batch, io);
    if (g.split.kslices > 1 && io.slab == nullptr)
        return fail(DAD_E_WORKSPACE, "%s: split-K launch without scratch", op.name.c_str());
    static const bool trace = getenv("DAD_TRACE_TILES") != nullptr;     // tuning aid
    if (trace)
        fprintf(stderr, "[dad] %-34s B=%d M=%d K=%dx%d L=%d tile=%d (%dx%d SK%d) kslices=%d%s\n", op.name.c_str(),
                batch, op.M, op.taps, op.cin0 + op.cin1, op.Lout, g.cfg, kTiles[g.cfg].BM, kTiles[g.cfg].BN,
                kTiles[g.cfg].SK, g.split.kslices, g.fused ? " +res1x1" : "");
#ifdef DAD_STAMPS
    p.stamps = (g_stamps && &op >= &m->plan.convs[0] && &op < &m->plan.convs[0] + m->plan.convs.size())
                   ? g_stamps + (size_t)(&op - &m->plan.convs[0]) * 4096 * 8 : nullptr;
#endif
    if (g.halo8) {                     // conv_halo8.hpp: same tile, grid, LDS and operands, its own slot shifts
        const void* fn = find_kernel(FAM_HALO8, {g.cfg, g.fused});
        if (fn != nullptr && g.halo8w) fn = find_halo8w(g.cfg, g.fused);      // the register-weight form: its own LDS size
        if (fn == nullptr || gn_pass || p.pre != nullptr || p.stats != nullptr || p.kslices != 1)
            return fail(DAD_E_INVALID, "no halo-skipping kernel for %s (tile %d res=%d wreg=%d)", op.name.c_str(), g.cfg, (int)g.fused, (int)g.halo8w);
        p.xswz = g.xswz8;
        void* hargs[] = {&p};
        HIP_TRY(hipLaunchKernel(fn, dim3(g.gx, g.gy, g.gz), dim3(g.threads), hargs, g.halo8w ? g.lds8w_bytes : g.lds_bytes, st));
        return DAD_OK;
    }
    const void* fn = find_kernel(FAM_GEMM, {g.cfg, op.taps, op.stride, launch_flags(op, g)});
    if (fn == nullptr)
        return fail(DAD_E_INVALID, "no kernel for %s (tile %d taps=%d stride=%d x3=%d bdir=%d ragged=%d res=%d)",
                    op.name.c_str(), g.cfg, op.taps, op.stride, (int)op.x3, (int)op.bdir, (int)g.ragged, (int)g.fused);
    void* args[] = {&p};
    HIP_TRY(hipLaunchKernel(fn, dim3(g.gx, g.gy, g.gz), dim3(g.threads), args, g.lds_bytes, st));
    if (gn_pass) return launch_gn_pass(m, op, g.gn_npt, batch, io, st);
    return DAD_OK;
}

int build_time_tables(dad_model* m, hipStream_t st);
// device copy of the two q_sample schedule vectors (the model's own allocation, freed with the others).  A load after
// dad_model_finalize overwrites the copy a step in flight may still read: the device is drained first.
int upload_train_schedule(dad_model* m) {
    const size_t T = m->train_sched[0].size();
    if (m->d_train_sched != nullptr) HIP_TRY(hipDeviceSynchronize());
    if (m->d_train_sched == nullptr) {
        void* a = nullptr;
        HIP_TRY(hipMalloc(&a, 2 * T * sizeof(float)));
        m->owned.push_back(a);
        m->d_train_sched = (float*)a;
    }
    HIP_TRY(hipMemcpy(m->d_train_sched, m->train_sched[0].data(), T * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_train_sched + T, m->train_sched[1].data(), T * sizeof(float), hipMemcpyHostToDevice));
    return DAD_OK;
}
// device copy of the two schedule vectors predict_start_from_noise reads (the dynamics-aware objective's x0_hat), made on
// first use behind a dad_model_load_schedule; a later load drains the device first, as above.
int ensure_recip_schedule(dad_model* m) {
    if (!m->have_sched) return fail(DAD_E_STATE, "schedule not loaded (dad_model_load_schedule)");
    if (!m->recip_sched_stale) return DAD_OK;
    const size_t T = m->sched[0].size();
    if (m->d_recip_sched != nullptr) HIP_TRY(hipDeviceSynchronize());
    if (m->d_recip_sched == nullptr) {
        void* a = nullptr;
        HIP_TRY(hipMalloc(&a, 2 * T * sizeof(float)));
        m->owned.push_back(a);
        m->d_recip_sched = (float*)a;
    }
    HIP_TRY(hipMemcpy(m->d_recip_sched, m->sched[0].data(), T * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->d_recip_sched + T, m->sched[1].data(), T * sizeof(float), hipMemcpyHostToDevice));
    m->recip_sched_stale = false;
    return DAD_OK;
}
// The per-timestep tables follow the time-MLP tensors lazily (dad_model_refresh_weights marks them stale): every
// entry point that reads them calls this first, on the stream it launches on.
int ensure_tables(dad_model* m, hipStream_t st) {
    if (!m->tables_stale) return DAD_OK;
    const int rc = build_time_tables(m, st);
    if (rc == DAD_OK) m->tables_stale = false;
    return rc;
}

// Every refusal of a forward entry point, before its first launch; `f`: what the call then replays (plan_forward).
int check_ready(const dad_model* m, int batch, int t, size_t ws_bytes, bool small_ok, FwdPlan& f) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!m->finalized) return fail(DAD_E_STATE, "dad_model_finalize has not been called");
    if (batch <= 0) return fail(DAD_E_INVALID, "batch must be positive (got %d)", batch);
    if (t < 0 || t >= m->cfg.n_timesteps)
        return fail(DAD_E_RANGE, "index %d is out of bounds for the schedule of size %d", t,
                    m->cfg.n_timesteps);
    const int rc = plan_forward(*m, false, batch, small_ok, f);
    if (ws_bytes < f.bytes)
        return fail(DAD_E_WORKSPACE, "workspace has %zu bytes, batch %d needs %zu", ws_bytes, batch,
                    f.bytes);
    return rc;
}

// ------------------------------------------------------------------ small-batch (CC) launches
// The tensor `in` names, as the consumer must read it (conv_cc.hpp).
dad::CcSrc cc_source(dad_model* m, const CcPlan& cc, const CcInput& in, int channels, const float* xext,
                     float* ws, int batch, int t) {
    dad::CcSrc s{};
    auto buf = [&](int id) -> float* { return ws + m->plan.bufs[id].offset * (long)batch; };
    float* slabs = ws + m->plan.floats_per_sample * (long)batch;
    s.C = channels;
    if (in.kind == 1) { s.data = xext; s.rows = batch * m->cfg.horizon; return s; }
    if (in.kind == 2) { s.data = buf(in.buf); return s; }
    const ConvOp& q = m->plan.convs[in.producer];
    const CcOp& qo = cc.ops[in.producer];
    s.data = slabs + qo.oslab;
    s.nsl = qo.kslices;
    s.C = qo.out_cols;
    s.rows = qo.out_rows;
    s.bias = q.d_bias;
    if (!q.norm.empty()) { s.gamma = q.d_gamma; s.beta = q.d_beta; s.cpg = q.cout / 8; }
    if (q.temb_off >= 0) s.temb = m->d_temb_table + (long)t * m->plan.temb_width + q.temb_off;
    if (qo.res_kind == 1) s.res = xext;
    else if (qo.res_kind == 2) s.res = buf(qo.res_buf);
    else if (qo.res_kind == 3) {
        const CcOp& r = cc.ops[qo.res_ride];
        s.rslab = slabs + r.orslab; s.nrs = r.kslices; s.rbias = m->plan.convs[qo.res_ride].d_rbias;
    } else if (qo.res_kind == 4) {                        // the block's stand-alone 1x1 residual conv
        const CcOp& r = cc.ops[qo.res_ride];
        s.rslab = slabs + r.oslab; s.nrs = r.kslices; s.rbias = m->plan.convs[qo.res_ride].d_bias;
    }
    s.mat = buf(in.buf);
    return s;
}

int run_conv_cc(dad_model* m, const CcPlan& cc, int i, const float* xext, float* ws, int batch, int t,
                hipStream_t st) {
    const ConvOp& op = m->plan.convs[i];
    const CcOp& o = cc.ops[i];
    dad::CcParams p{};
    p.src0 = cc_source(m, cc, o.in0, op.cin0, xext, ws, batch, t);
    if (o.in1.kind != 0) p.src1 = cc_source(m, cc, o.in1, op.cin1, xext, ws, batch, t);
    p.w = op.d_w; p.wtaps = op.wtaps();
    p.cin0 = op.cin0; p.cin1 = op.cin1; p.M = op.M;
    p.B = batch; p.Lin = op.Lin; p.Lout = op.Lout;
    p.lshift = ilog2(op.Lout); p.lshift_in = ilog2(op.Lin);
    p.interleave = op.kind == CONV_UP;
    p.slice_ch = o.slice_ch;
    float* slabs = ws + m->plan.floats_per_sample * (long)batch;
    p.oslab = slabs + o.oslab;
    p.orslab = o.orslab >= 0 ? slabs + o.orslab : nullptr;
    p.out_rows = o.out_rows;
    const void* kern = o.wide ? find_kernel(FAM_CCW, {op.taps, op.stride, op.ride, o.ride_in, o.tile_rows})
                              : find_kernel(FAM_CC, {op.taps, op.stride, op.ride, o.big, o.tile_rows, op.Lout > 32});
    if (!kern) return fail(DAD_E_INVALID, "no small-batch kernel for %s (taps=%d stride=%d)", op.name.c_str(), op.taps, op.stride);
    static const bool trace = getenv("DAD_TRACE_TILES") != nullptr;
    if (trace)
        fprintf(stderr, "[dad] %-34s B=%d M=%d K=%dx%d L=%d cc slice=%d kslices=%d ntiles=%d%s\n", op.name.c_str(), batch,
                op.M, op.taps, op.cin0 + op.cin1, op.Lout, o.slice_ch, o.kslices, o.ntiles, op.ride ? " +res1x1" : "");
    if (trace && o.wide) fprintf(stderr, "[dad]   (wide: %d-row tiles, %zu B LDS)\n", o.tile_rows, o.lds_bytes);
#ifdef DAD_STAMPS
    p.stamps = g_stamps ? g_stamps + (size_t)i * 16 : nullptr;
#endif
    void* args[] = {&p};
    HIP_TRY(hipLaunchKernel(kern, dim3(o.kslices, op.M / 32, o.ntiles), dim3(dad::CC_THREADS), args, o.lds_bytes, st));
    return DAD_OK;
}

// The ancestral step at t of the loaded schedule (host_plan.hpp ancestral_coef)
dad_sampler_coef schedule_step(const dad_model* m, int t) {
    return ancestral_coef(t, m->sched[0][t], m->sched[1][t], m->sched[2][t], m->sched[3][t], m->sched[4][t]);
}

// final_conv[1] and the posterior update of step `s` on the trajectories x (dad_step_args `a`), as kernel parameters
void posterior_params(dad_model* m, const FwdPlan& f, float* x, const dad_sampler_coef& s, const dad_step_args* a,
                      int x_out_disabled, bool seed_from_device, float* ws, dad::FinalParams& p) {
    const dad_cfg& c = m->cfg;
    const Plan& plan = f.train ? m->tplan : m->plan;
    p.act = ws + plan.bufs[plan.final_act].offset * (long)f.batch;
    p.w = m->d_final_w; p.bias = m->d_final_b;
    p.dim = c.dim; p.td = c.transition_dim; p.B = f.batch; p.H = traj_horizon(*m); p.Hact = c.horizon;
    p.predict_epsilon = c.predict_epsilon; p.clip_denoised = c.clip_denoised;
    p.x = x;
    p.noise = a->noise; p.cond0 = a->cond0; p.cond_per_row = a->cond_per_row;
    p.guide = (a->guide_grad && a->guide_weight > 0.0f) ? a->guide_grad : nullptr;
    p.mean_out = a->mean_out; p.eps_out = a->eps_out;
    p.x_out_disabled = x_out_disabled;
    p.c_recip = s.c_recip; p.c_recipm1 = s.c_recipm1;
    p.coef1 = s.coef_x0; p.coef2 = s.coef_xt;
    p.sigma = s.sigma;
    p.guide_scale = a->guide_weight * s.guide_mean;
    p.guide_x0 = a->guide_weight * s.guide_x0;
    p.seed = a->seed;
    p.elem_offset = a->row_offset * (uint64_t)traj_horizon(*m) * (uint64_t)c.transition_dim;
    p.draw = a->draw;
    p.seed_dev = seed_from_device ? (const unsigned long long*)m->d_rng : nullptr;
}

// The seam of the sampling loop (conv_seam.hpp, plan_seam): the posterior update of one step and, on the new x, the
// first launch of the next step's evaluation.
struct SeamCall {
    const SeamPlan* plan;
    float* x;
    const dad_sampler_coef* s;   // the step whose posterior update the launch carries
    const dad_step_args* a;      //   and its arguments
    bool seed_from_device;
};
int launch_seam(dad_model* m, const FwdPlan& f, const SeamCall& sc, int t_conv, float* ws, hipStream_t st) {
    const FwdLaunch& l = f.launches[0];
    const ConvOp& op = m->plan.convs[l.conv];
    dad::SeamParams q{};
    posterior_params(m, f, sc.x, *sc.s, sc.a, 0, sc.seed_from_device, ws, q.f);
    q.c = conv_params(m, op, l.g, f.batch, conv_io(m, f, l, sc.x, ws, t_conv, nullptr, nullptr));
    q.c.xswz = sc.plan->xswz;
    q.units = sc.plan->units;
    q.hshift = ilog2(m->cfg.horizon);
    const void* fn = find_kernel(FAM_SEAM, {m->cfg.dim, sc.plan->tile0});
    if (fn == nullptr || q.c.rdst == nullptr || q.c.rbias == nullptr || q.c.gamma == nullptr)
        return fail(DAD_E_INVALID, "no seam kernel for dim %d on tile %d", m->cfg.dim, sc.plan->cfg);
    void* args[] = {&q};
    HIP_TRY(hipLaunchKernel(fn, dim3(sc.plan->grid), dim3(sc.plan->threads), args, sc.plan->lds_bytes, st));
    return DAD_OK;
}

// A library guide (guide_mlp.hpp) on trajectories of one shape: what dad_guide_grad and dad_guided_loop check before
// anything is launched, and the launch itself.
static_assert(dad::GUIDE_TANH == DAD_GD_TANH && dad::GUIDE_RELU == DAD_GD_RELU && dad::GUIDE_MISH == DAD_GD_MISH, "DAD_GD_ACTS");
static_assert(dad::GM_MAX_LAYERS == DAD_GUIDE_MAX_LAYERS, "dad_guide_args");
struct GuideCall {
    dad::GuideParams p;
    int activation;
    GuidePlan plan;
};
int guide_call_checked(const dad_guide_args* g, const float* x, float* grad, float* value_rows, int batch, int horizon,
                       int td, GuideCall& c) {
    if (!g) return fail(DAD_E_INVALID, "guide: arguments missing");
    if (!x || !grad) return fail(DAD_E_INVALID, "guide: null pointer");
    int rc = guide_shape_checked(batch, horizon, td);
    if (rc != DAD_OK) return rc;
    const int L = g->n_layers;
    c.plan = plan_guide(g->in_dim, L >= 0 && L <= DAD_GUIDE_MAX_LAYERS ? g->widths : nullptr, L, g->activation, batch, horizon, td);
    if (c.plan.refused != DAD_GD_OK)
        return fail(DAD_E_INVALID, "guide refused (%d layers, in_dim=%d, transition_dim=%d, activation=%d): %s", L, g->in_dim,
                    td, g->activation, guide_refusal(c.plan.refused));
    for (int i = 0; i < L; ++i)
        if (g->padded[i] != c.plan.padded[i])
            return fail(DAD_E_INVALID, "guide: padded[%d]=%d, the plan pads it to %d (dad_debug_guide_plan)", i, g->padded[i],
                        c.plan.padded[i]);
    for (int i = 0; i < L; ++i)
        if (!g->w_fwd[i] || !g->bias[i] || (i + 1 < L && !g->w_bwd[i]))
            return fail(DAD_E_INVALID, "guide: layer %d has a null weight image or bias", i);
    dad::GuideParams& p = c.p;
    p = dad::GuideParams{};
    p.x = x; p.grad = grad; p.value_rows = value_rows;
    for (int i = 0; i + 1 < L; ++i) { p.wf[i] = g->w_fwd[i]; p.wb[i] = g->w_bwd[i]; p.bias[i] = g->bias[i]; }
    p.w_last = g->w_fwd[L - 1]; p.b_last = g->bias[L - 1];
    p.rows = batch * horizon; p.td = td; p.in_dim = g->in_dim; p.hidden = L - 1;
    for (int i = 0; i < L; ++i) p.pad[i] = c.plan.padded[i];
    c.activation = g->activation;
    return DAD_OK;
}
int launch_guide(const GuideCall& c, hipStream_t st) {
    const dim3 grid(c.plan.gx), block(c.plan.threads);
    switch (c.activation) {
        case DAD_GD_TANH: hipLaunchKernelGGL(dad::guide_mlp_kernel<dad::GUIDE_TANH>, grid, block, c.plan.lds_bytes, st, c.p); break;
        case DAD_GD_RELU: hipLaunchKernelGGL(dad::guide_mlp_kernel<dad::GUIDE_RELU>, grid, block, c.plan.lds_bytes, st, c.p); break;
        default: hipLaunchKernelGGL(dad::guide_mlp_kernel<dad::GUIDE_MISH>, grid, block, c.plan.lds_bytes, st, c.p); break;
    }
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

// One denoiser evaluation up to final_conv[0]: the launches of `f`, nothing else.  `seam`: the first of them goes out
// as the seam launch, which also carries the previous step's posterior update (counted as that first launch)
// `guide`: the launch of a library guide on x goes out after the evaluation's first launch — after the seam launch where
// there is one: it reads the previous step's gradient and writes the x this step's guide is taken at.
int run_unet(dad_model* m, const FwdPlan& f, const float* x, int t, float* ws, hipStream_t st,
             const int32_t* trow = nullptr, const float* temb_rows = nullptr, const SeamCall* seam = nullptr,
             const GuideCall* guide = nullptr) {
    // Profiling brackets the whole run of conv-GEMM launches of one denoiser evaluation with
    // ONE pair of HIP events on the launch stream (events between individual launches would
    // break the back-to-back dispatch they are meant to time).
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (m->profile) {
        if (m->ev_used == m->ev_pool.size()) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            m->ev_pool.push_back({a, b});
        }
        e0 = m->ev_pool[m->ev_used].first;
        e1 = m->ev_pool[m->ev_used].second;
        ++m->ev_used;
        HIP_TRY(hipEventRecord(e0, st));
    }
    bool guide_due = guide != nullptr;
    for (size_t i = 0; f.cc.ok && i < f.cc.ops.size(); ++i) {        // small batch: consumer-combine kernels
        if (!f.cc.ops[i].launched) continue;
        int rc = run_conv_cc(m, f.cc, (int)i, x, ws, f.batch, t, st);
        if (rc != DAD_OK) return rc;
        if (guide_due && seam == nullptr) {
            guide_due = false;
            if ((rc = launch_guide(*guide, st)) != DAD_OK) return rc;
        }
    }
    for (const FwdLaunch& l : f.launches) {
        const bool seam_launch = seam != nullptr && &l == &f.launches[0];
        int rc = seam_launch ? launch_seam(m, f, *seam, t, ws, st) : run_conv(m, f, l, x, ws, t, st, trow, temb_rows);
        if (rc != DAD_OK) return rc;
        if (guide_due && (seam == nullptr || seam_launch)) {
            guide_due = false;
            if ((rc = launch_guide(*guide, st)) != DAD_OK) return rc;
        }
    }
    if (m->profile) {                 // (a riding 1x1 residual conv counts its flops, not a launch)
        for (const ConvOp& op : m->plan.convs) m->prof_flops += op.flops_per_sample * f.batch;
        for (const CcOp& o : f.cc.ops) m->prof_launches += o.launched;
        m->prof_launches += (int64_t)f.launches.size();
        HIP_TRY(hipEventRecord(e1, st));
    }
    return DAD_OK;
}

// final_conv[1] and the posterior update (or, `eps_only`, the network output alone), on the grid `f` planned
int run_final(dad_model* m, const FwdPlan& f, float* x, const float* x_ro, int t, const dad_sampler_coef* s,
              const dad_step_args* a, int x_out_disabled, float* eps_only, float* ws, hipStream_t st,
              bool seed_from_device = false) {
    const dad_cfg& c = m->cfg;
    const int batch = f.batch;
    dad::FinalParams p{};
    const Plan& plan = f.train ? m->tplan : m->plan;
    p.act = ws + plan.bufs[plan.final_act].offset * (long)batch;
    p.w = m->d_final_w; p.bias = m->d_final_b;
    p.dim = c.dim; p.td = c.transition_dim; p.B = batch; p.H = traj_horizon(*m); p.Hact = c.horizon;
    p.predict_epsilon = c.predict_epsilon; p.clip_denoised = c.clip_denoised;
    if (eps_only) {
        p.x = const_cast<float*>(x_ro);
        p.eps_out = eps_only;
        p.x_out_disabled = 1;
    } else {
        posterior_params(m, f, x, *s, a, x_out_disabled, seed_from_device, ws, p);
    }
    const dim3 grid(f.final_gx, f.final_gy);
    if (f.cc.ok) {
        dad::FinalCcParams fp{};
        CcInput in; in.kind = 3; in.producer = f.cc.final_producer; in.buf = m->plan.final_act;
        fp.src = cc_source(m, f.cc, in, c.dim, x_ro ? x_ro : x, ws, batch, t);
        fp.src.mat = nullptr;
        fp.f = p;
        hipLaunchKernelGGL(dad::final_cc_kernel, grid, dim3(dad::CC_THREADS), f.final_lds, st, fp);
    } else {
        hipLaunchKernelGGL(dad::final_posterior_kernel, grid, dim3(256), f.final_lds, st, p);
    }
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

int run_project(const dad_project_args* pa, float alpha, float* x, int batch, int horizon,
                hipStream_t st, float* violation = nullptr) {
    if (!pa || !pa->P) return fail(DAD_E_INVALID, "projection arguments missing");
    if (alpha <= 0.0f && !violation) return DAD_OK;       // policies.py:428-429
    {
        const int rc0 = configure_kernels();
        if (rc0 != DAD_OK) return rc0;
    }
    dad::ProjParams p{};
    p.P = pa->P; p.obs_mean = pa->obs_mean; p.obs_std = pa->obs_std;
    p.act_mean = pa->act_mean; p.act_std = pa->act_std;
    p.x = x; p.B = batch; p.H = horizon; p.n = pa->state_dim; p.od = pa->observation_dim;
    p.m = pa->action_dim;
    p.D = (horizon + 1) * p.n + horizon * p.m;
    p.alpha = alpha;
    p.one_minus_alpha = (float)(1.0 - (double)alpha);
    p.violation = violation;
    const size_t x_bytes = (size_t)batch * horizon * (pa->observation_dim + pa->action_dim) * sizeof(float);
    const ProjectPlan q = plan_project(p.D, batch, x_bytes, pa->scratch ? pa->scratch_bytes : 0, violation != nullptr);
    if (q.refused)
        return fail(DAD_E_INVALID, "projection dimension D=%d: one trajectory's partial sums exceed LDS; pass "
                    "dad_project_args.scratch and a batch of at least 32 for the GEMM form", p.D);
    const dim3 grid(q.gx, q.gy);
    if (q.form == DAD_PP_GEMM) {
        p.xout = pa->scratch;
        hipLaunchKernelGGL(dad::project_gemm_kernel, grid, dim3(dad::PG_THREADS), q.lds_bytes, st, p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(x, pa->scratch, x_bytes, hipMemcpyDeviceToDevice, st));
        return DAD_OK;
    }
    p.xout = x;
    if (q.form == DAD_PP_ROW1)
        hipLaunchKernelGGL((dad::project_kernel<1, dad::PROJ_KP>), grid, dim3(64 * dad::PROJ_KP), q.lds_bytes, st, p);
    else
        hipLaunchKernelGGL((dad::project_kernel<4, dad::PROJ_KP>), grid, dim3(64 * dad::PROJ_KP), q.lds_bytes, st, p);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

// What the two passes of the violation gradient check before anything touches the device, and the plan they launch from.
int violation_grad_plan_of(const dad_project_args* pa, const void* workspace, size_t workspace_bytes, int batch, int horizon,
                           int form, int& D, ViolationGradPlan& q) {
    if (!pa || !pa->P || !pa->obs_mean || !pa->obs_std || !pa->act_mean || !pa->act_std)
        return fail(DAD_E_INVALID, "violation gradient: projection arguments missing");
    if (!workspace) return fail(DAD_E_INVALID, "violation gradient: null workspace");
    const int rc = violation_grad_plan_checked(pa->state_dim, pa->observation_dim, pa->action_dim, batch, horizon, form, D, q);
    if (rc != DAD_OK) return rc;
    if (q.refused)
        return fail(DAD_E_INVALID, "violation gradient: the row form at D=%d needs %zu bytes of LDS for one trajectory and its partial "
                    "sums (a CU has %zu); the GEMM form (form 1, or -1) takes any D", D, q.fwd.lds_bytes, dad::kLdsBytes);
    if (workspace_bytes < q.workspace_bytes)
        return fail(DAD_E_WORKSPACE, "violation gradient: workspace of %zu bytes, %zu needed (dad_violation_grad_workspace_bytes)",
                    workspace_bytes, q.workspace_bytes);
    return DAD_OK;
}

int run_violation_fwd(const dad_project_args* pa, const float* x, float* violation, void* workspace, size_t workspace_bytes,
                      int batch, int horizon, int form, hipStream_t st) {
    if (!x || !violation) return fail(DAD_E_INVALID, "violation gradient: null pointer");
    int D = 0;
    ViolationGradPlan q;
    int rc = violation_grad_plan_of(pa, workspace, workspace_bytes, batch, horizon, form, D, q);
    if (rc != DAD_OK || (rc = configure_kernels()) != DAD_OK) return rc;
    float* const ws = (float*)workspace;
    dad::ViolationFwdParams f{};
    dad::ProjParams& p = f.proj;
    p.P = pa->P; p.obs_mean = pa->obs_mean; p.obs_std = pa->obs_std; p.act_mean = pa->act_mean; p.act_std = pa->act_std;
    p.x = const_cast<float*>(x); p.xout = nullptr;
    p.B = batch; p.H = horizon; p.n = pa->state_dim; p.od = pa->observation_dim; p.m = pa->action_dim; p.D = D;
    p.alpha = 1.0f; p.one_minus_alpha = 0.0f;
    p.violation = violation;
    p.resid = ws + q.r_off;
    const dim3 grid(q.fwd.gx, q.fwd.gy);
    if (q.form == DAD_VG_ROW) {
        if (q.fwd.rows_per_block == 1)
            hipLaunchKernelGGL((dad::project_kernel<1, dad::PROJ_KP>), grid, dim3(64 * dad::PROJ_KP), q.fwd.lds_bytes, st, p);
        else
            hipLaunchKernelGGL((dad::project_kernel<4, dad::PROJ_KP>), grid, dim3(64 * dad::PROJ_KP), q.fwd.lds_bytes, st, p);
        HIP_TRY(hipGetLastError());
        return DAD_OK;
    }
    f.part = ws + q.part_off;
    f.col_blocks = q.col_blocks;
    hipLaunchKernelGGL(dad::violation_fwd_gemm_kernel, grid, dim3(dad::PG_THREADS), q.fwd.lds_bytes, st, f);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dad::violation_sum_kernel, dim3(q.fwd.tail_gx), dim3(dad::VG_TAIL_THREADS), 0, st,
                       (const float*)f.part, violation, batch, q.col_blocks);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

int run_violation_bwd(const dad_project_args* pa, const float* d_violation, float* d_x, void* workspace, size_t workspace_bytes,
                      int batch, int horizon, int form, hipStream_t st) {
    if (!d_violation || !d_x) return fail(DAD_E_INVALID, "violation gradient: null pointer");
    int D = 0;
    ViolationGradPlan q;
    int rc = violation_grad_plan_of(pa, workspace, workspace_bytes, batch, horizon, form, D, q);
    if (rc != DAD_OK || (rc = configure_kernels()) != DAD_OK) return rc;
    float* const ws = (float*)workspace;
    dad::ViolationBwdParams p{};
    p.P = pa->P; p.obs_std = pa->obs_std; p.act_std = pa->act_std;
    p.r = ws + q.r_off; p.w = d_violation; p.g = ws + q.g_off; p.dx = d_x;
    p.B = batch; p.H = horizon; p.n = pa->state_dim; p.od = pa->observation_dim; p.m = pa->action_dim; p.D = D;
    p.row_elems = horizon * (pa->observation_dim + pa->action_dim);
    const dim3 grid(q.bwd.gx, q.bwd.gy);
    if (q.form == DAD_VG_ROW) {
        hipLaunchKernelGGL(dad::violation_bwd_row_kernel, grid, dim3(64 * dad::VG_ROW_WAVES), q.bwd.lds_bytes, st, p);
        HIP_TRY(hipGetLastError());
        return DAD_OK;
    }
    hipLaunchKernelGGL(dad::violation_bwd_gemm_kernel, grid, dim3(dad::PG_THREADS), q.bwd.lds_bytes, st, p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dad::violation_scatter_kernel, dim3(q.bwd.tail_gx), dim3(dad::VG_TAIL_THREADS), 0, st, p);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

// One reverse step `s` (already checked) on the plan `f`: the body of dad_denoise_step and dad_sampler_step
int sampler_step(dad_model* m, const FwdPlan& f, float* x, const dad_sampler_coef& s, const dad_step_args* args,
                 int x_out_disabled, void* workspace, dad_stream_t stream) {
    if (!x || !args || !workspace) return fail(DAD_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = ensure_tables(m, st)) != DAD_OK) return rc;
    if ((rc = run_unet(m, f, x, s.t, (float*)workspace, st)) != DAD_OK) return rc;
    return run_final(m, f, x, nullptr, s.t, &s, args, x_out_disabled, nullptr, (float*)workspace, st);
}

// The sampling loop over `n_steps` checked steps in execution order (proj_alphas likewise), on the plan `f`: the body
// of dad_sample_loop and dad_sampler_loop, and the one place a loop is captured and replayed.
int sampler_loop(dad_model* m, const FwdPlan& f, float* x, const dad_sampler_coef* steps, int n_steps, int batch,
                 const float* noise_stack, uint64_t seed, uint64_t row_offset, const float* cond0, int cond_per_row,
                 const dad_project_args* proj, const float* proj_alphas, int use_graph, void* workspace,
                 dad_stream_t stream, const dad_guide_args* guide = nullptr, float guide_weight = 0.0f) {
    int rc;
    if (!x || !workspace) return fail(DAD_E_INVALID, "null pointer");
    if (proj && !proj_alphas) return fail(DAD_E_INVALID, "projection needs per-step alphas");
    // a library guide: its launch per iteration writes guide->grad, which the step's tail (or the seam that carries it) reads
    const bool guided = guide != nullptr && guide_weight > 0.0f;
    GuideCall gc;
    if (guided) {
        const long need = (long)batch * traj_horizon(*m) * m->cfg.transition_dim * (long)sizeof(float);
        if (!guide->grad || (long)std::min<size_t>(guide->grad_bytes, (size_t)INT64_MAX) < need)
            return fail(DAD_E_INVALID, "guide: dad_guide_args.grad must hold batch * H * td = %ld bytes (got %zu)", need,
                        guide->grad ? guide->grad_bytes : (size_t)0);
        if ((rc = guide_call_checked(guide, x, guide->grad, nullptr, batch, traj_horizon(*m), m->cfg.transition_dim, gc)) != DAD_OK)
            return rc;
        if ((rc = configure_kernels()) != DAD_OK) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_tables(m, st)) != DAD_OK) return rc;      // (before any capture: the replayed loop reads the tables)
    const long step_elems = (long)batch * traj_horizon(*m) * m->cfg.transition_dim;

    const bool seed_dev = use_graph && !m->profile && noise_stack == nullptr;
    // The seam between two steps as one launch (plan_seam): iteration 0 runs the whole evaluation, every later one starts
    // with the seam launch — the previous step's posterior update and this evaluation's first conv — and the last
    // step ends with the posterior launch.
    const SeamPlan seam = plan_seam(*m, f, proj != nullptr);
    const bool seamed = seam.taken() && n_steps > 1;
    auto enqueue_all = [&](hipStream_t st) -> int {
        dad_step_args prev{};
        for (int j = 0; j < n_steps; ++j) {
            const int t = steps[j].t;
            dad_step_args a{};
            a.noise = noise_stack ? noise_stack + (long)j * step_elems : nullptr;
            a.seed = seed; a.row_offset = row_offset; a.draw = (uint64_t)(j + 1);
            a.cond0 = cond0; a.cond_per_row = cond_per_row;
            if (guided) { a.guide_grad = guide->grad; a.guide_weight = guide_weight; }
            const SeamCall sc{&seam, x, j > 0 ? &steps[j - 1] : nullptr, &prev, seed_dev};
            int r = run_unet(m, f, x, t, (float*)workspace, st, nullptr, nullptr, seamed && j > 0 ? &sc : nullptr,
                             guided ? &gc : nullptr);
            if (r != DAD_OK) return r;
            prev = a;
            if (seamed && j + 1 < n_steps) continue;
            if ((r = run_final(m, f, x, nullptr, t, &steps[j], &a, 0, nullptr, (float*)workspace, st, seed_dev)) != DAD_OK) return r;
            if (proj && (r = run_project(proj, proj_alphas[j], x, batch, traj_horizon(*m), st)) != DAD_OK)
                return r;
        }
        return DAD_OK;
    };

    if (!use_graph || m->profile) return enqueue_all(st);

    // Graph replay: the whole loop is one hipGraph keyed by every frozen pointer and scalar (the
    // steps' coefficients by their hash).  With in-kernel noise the Philox key is read from device
    // memory, written by a tiny kernel ahead of the replay, so a new seed does not need a new capture.
    if (seed_dev) {
        hipLaunchKernelGGL(dad::set_u64_kernel, dim3(1), dim3(1), 0, st,
                           (unsigned long long*)m->d_rng, (unsigned long long)seed);
        HIP_TRY(hipGetLastError());
    }
    GraphKey key{};
    key.x = x; key.noise = noise_stack; key.cond = cond0; key.ws = workspace;
    if (proj) {
        key.P = proj->P; key.obs_mean = proj->obs_mean; key.obs_std = proj->obs_std;
        key.act_mean = proj->act_mean; key.act_std = proj->act_std;
        key.proj_scratch = proj->scratch;
        key.state_dim = proj->state_dim; key.observation_dim = proj->observation_dim;
        key.action_dim = proj->action_dim;
    }
    if (guided) {
        for (int i = 0; i < guide->n_layers; ++i) {
            key.guide_ptrs[3 * i] = guide->w_fwd[i]; key.guide_ptrs[3 * i + 1] = guide->w_bwd[i];
            key.guide_ptrs[3 * i + 2] = guide->bias[i];
            key.guide_shape[3 + i] = guide->widths[i]; key.guide_shape[3 + DAD_GUIDE_MAX_LAYERS + i] = guide->padded[i];
        }
        key.guide_ptrs[3 * DAD_GUIDE_MAX_LAYERS] = guide->grad;
        key.guide_shape[0] = guide->n_layers; key.guide_shape[1] = guide->in_dim; key.guide_shape[2] = guide->activation;
        key.guide_weight = guide_weight;
    }
    key.n_steps = n_steps; key.batch = batch; key.cond_per_row = cond_per_row;
    key.force_tile = m->force_tile;
    key.flags = (m->split_enabled ? 1 : 0) | (m->fuse_residual ? 2 : 0) | (m->xswz_enabled ? 4 : 0) |
                (m->xcd_order ? 8 : 0) | (f.cc.ok ? 16 : 0) | (m->step_seam ? 32 : 0) | ((m->halo8_wreg + 1) << 6) | (m->split_target << 8);
    key.row_offset = row_offset;
    if (proj) key.alpha_hash = fnv1a_bytes(proj_alphas, (size_t)n_steps * sizeof(float));
    key.steps_hash = sampler_steps_hash(steps, n_steps);
    auto it = m->graphs.find(key);
    if (it == m->graphs.end()) {
        if (m->graphs.size() >= 16) {                 // bounded cache: drop everything, re-capture
            // a replay may still be in flight on the caller's stream (or on another one the caller
            // used earlier): wait for the device before destroying executable graphs
            HIP_TRY(hipDeviceSynchronize());
            for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
            m->graphs.clear();
        }
        // capture on a private stream: the caller's stream may be the null stream, which
        // cannot be captured; nothing executes during capture.
        if (!m->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeRelaxed));
        rc = enqueue_all(m->cap_stream);
        hipError_t e = hipStreamEndCapture(m->cap_stream, &graph);
        if (rc != DAD_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess) return fail(DAD_E_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        hipGraphExec_t exec = nullptr;
        e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) return fail(DAD_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
        it = m->graphs.emplace(key, exec).first;
    }
    HIP_TRY(hipGraphLaunch(it->second, st));
    return DAD_OK;
}

// Per-timestep tables from the device copies of the time-MLP tensors: time_mlp (Linear -> Mish -> Linear
// on the sinusoid rows) and every block's Mish -> Linear (temporal_unet.py:97-100,155-160).
int build_time_tables(dad_model* m, hipStream_t st) {
    const dad_cfg& c = m->cfg;
    const int T = c.n_timesteps, dim = c.dim, tdm = c.time_dim;
    auto linear = [&](const float* in, const std::string& key, float* out, int K, int M, int stride, int mish_in) -> int {
        auto w = m->d_time.find(key + ".weight"), b = m->d_time.find(key + ".bias");
        if (w == m->d_time.end() || b == m->d_time.end()) return fail(DAD_E_KEY, "missing key '%s'", key.c_str());
        const long total = (long)T * M;
        hipLaunchKernelGGL(dad::table_linear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256),
                           0, st, in, w->second, b->second, out, T, K, M, stride, mish_in);
        HIP_TRY(hipGetLastError());
        return DAD_OK;
    };
    int rc;
    if ((rc = linear(m->d_emb, "time_mlp.1", m->d_h1, dim, 4 * tdm, 4 * tdm, 0)) != DAD_OK) return rc;
    if ((rc = linear(m->d_h1, "time_mlp.3", m->d_temb, 4 * tdm, tdm, tdm, 1)) != DAD_OK) return rc;
    for (const ConvOp& op : m->plan.convs) {
        if (op.temb_off < 0) continue;
        std::string base = op.name.substr(0, op.name.size() - std::strlen(".blocks.0.block.0"));
        if ((rc = linear(m->d_temb, base + ".time_mlp.1", m->d_temb_table + op.temb_off, tdm, op.cout,
                         m->plan.temb_width, 1)) != DAD_OK) return rc;
    }
    return DAD_OK;
}

}  // namespace

// ===================================================================================== ABI
extern "C" {

const char* dad_last_error(void) { return g_err; }
const char* dad_version(void) { return "dad-hip 0.1 (gfx950, fp32 MFMA)"; }

int dad_model_create(const dad_cfg* cfg, dad_model** out) {
    if (!cfg || !out) return fail(DAD_E_INVALID, "null argument");
    int rc = check_cfg(cfg);
    if (rc != DAD_OK) return rc;
    std::unique_ptr<dad_model> m(new dad_model());
    m->cfg = *cfg;
    // A/B switches for tuning runs (read once, per model)
    m->xswz_enabled = getenv("DAD_NO_XSWZ") == nullptr;
    m->xcd_order = getenv("DAD_NO_XCD_ORDER") == nullptr;
    m->fuse_residual = getenv("DAD_NO_FUSE_RES") == nullptr;
    if (const char* v = getenv("DAD_SPLIT_TARGET")) m->split_target = std::max(1, atoi(v));
    m->cc_enabled = getenv("DAD_NO_CC") == nullptr;
    if (const char* v = getenv("DAD_CC_MAX_ROWS")) m->cc_max_rows = std::max(0, atoi(v));
    if (const char* v = getenv("DAD_WGRAD_BLOCKS")) m->wgrad_blocks = std::max(1, atoi(v));
    if ((rc = build_plan(m.get())) != DAD_OK) return rc;
    *out = m.release();
    return DAD_OK;
}

void dad_model_destroy(dad_model* m) {
    if (!m) return;
    free_device(m);
    if (m->cap_stream) (void)hipStreamDestroy(m->cap_stream);
    for (auto& e : m->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    delete m;
}

int dad_model_load_weight(dad_model* m, const char* key, const float* data, const int64_t* shape,
                          int32_t ndim) {
    if (!m || !key || !data || !shape) return fail(DAD_E_INVALID, "null argument");
    auto it = m->expected.find(key);
    if (it == m->expected.end()) return fail(DAD_E_KEY, "unexpected key '%s'", key);
    if ((int)it->second.size() != ndim) return fail(DAD_E_KEY, "'%s': rank %d, expected %zu", key, ndim, it->second.size());
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] != it->second[i])
            return fail(DAD_E_KEY, "'%s': size mismatch at dim %d (%lld vs %lld)", key, i,
                        (long long)shape[i], (long long)it->second[i]);
        n *= (size_t)shape[i];
    }
    HostTensor& t = m->raw[key];
    t.shape.assign(shape, shape + ndim);
    t.data.assign(data, data + n);
    m->finalized = false;
    return DAD_OK;
}

int dad_model_load_schedule(dad_model* m, const float* a, const float* b, const float* c1,
                            const float* c2, const float* lv) {
    if (!m || !a || !b || !c1 || !c2 || !lv) return fail(DAD_E_INVALID, "null argument");
    const float* src[5] = {a, b, c1, c2, lv};
    for (int i = 0; i < 5; ++i) m->sched[i].assign(src[i], src[i] + m->cfg.n_timesteps);
    m->have_sched = true;
    m->recip_sched_stale = true;
    return DAD_OK;
}

int dad_model_load_train_schedule(dad_model* m, const float* sqrt_ac, const float* sqrt_1m_ac, int32_t n) {
    if (!m || !sqrt_ac || !sqrt_1m_ac) return fail(DAD_E_INVALID, "null argument");
    if (n != m->cfg.n_timesteps)
        return fail(DAD_E_INVALID, "training schedule has %d entries, the model %d timesteps", n, m->cfg.n_timesteps);
    m->train_sched[0].assign(sqrt_ac, sqrt_ac + n);
    m->train_sched[1].assign(sqrt_1m_ac, sqrt_1m_ac + n);
    return m->finalized ? upload_train_schedule(m) : DAD_OK;
}

int dad_model_load_time_embedding(dad_model* m, const float* emb, int32_t n_timesteps, int32_t dim) {
    if (!m || !emb) return fail(DAD_E_INVALID, "null argument");
    if (n_timesteps != m->cfg.n_timesteps || dim != m->cfg.dim)
        return fail(DAD_E_INVALID, "time embedding must be (%d, %d), got (%d, %d)", m->cfg.n_timesteps,
                    m->cfg.dim, n_timesteps, dim);
    m->emb_override.assign(emb, emb + (size_t)n_timesteps * dim);
    m->finalized = false;
    return DAD_OK;
}

int dad_model_set_precision(dad_model* m, int32_t precision) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (precision != DAD_PREC_FP32 && precision != DAD_PREC_F16X3)
        return fail(DAD_E_INVALID, "unknown precision %d (DAD_PREC_FP32 = 0, DAD_PREC_F16X3 = 1)", precision);
    if (precision != m->precision) m->finalized = false;       // weights must be re-packed
    m->precision = precision;
    decide_kernel_families(m);
    return DAD_OK;
}

int dad_model_set_horizon(dad_model* m, int32_t real_horizon) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    const int padded = m->cfg.horizon, down = 1 << (m->cfg.n_levels - 1);
    if (real_horizon < down || real_horizon > padded || real_horizon % down != 0)
        return fail(DAD_E_INVALID, "horizon %d: need a multiple of 2^(levels-1) = %d (every level halves the length) of at most the "
                    "padded horizon %d", real_horizon, down, padded);
    m->real_horizon = real_horizon == padded ? 0 : real_horizon;
    const int rc = build_plan(m);                 // the same plan; every conv now knows how many of its rows exist
    if (rc != DAD_OK) return rc;
    m->finalized = false;
    if (m->training) if (const char* why = training_refusal(*m)) return fail(DAD_E_INVALID, "training: %s", why);
    return DAD_OK;
}

int dad_model_set_group_channels(dad_model* m, const int32_t* real_channels, int32_t n_levels) {
    if (!m || !real_channels) return fail(DAD_E_INVALID, "null argument");
    if (n_levels != m->cfg.n_levels) return fail(DAD_E_INVALID, "%d levels given, the model has %d", n_levels, m->cfg.n_levels);
    for (int i = 0; i < n_levels; ++i) {
        const int real = real_channels[i], padded = m->cfg.channels[i];
        if (real < 8 || real % 8 != 0 || real > padded)
            return fail(DAD_E_INVALID, "level %d: %d real channels in %d (need a multiple of 8, at most the padded width)", i, real, padded);
    }
    for (int i = 0; i < DAD_MAX_LEVELS; ++i) m->real_channels[i] = i < n_levels ? real_channels[i] : 0;
    const int rc = build_plan(m);                 // the same plan; every GroupNorm'd conv now knows its real group width
    if (rc != DAD_OK) return rc;
    m->finalized = false;
    if (m->training) if (const char* why = training_refusal(*m)) return fail(DAD_E_INVALID, "training: %s", why);
    return DAD_OK;
}

int dad_model_finalize(dad_model* m, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!m->have_sched) return fail(DAD_E_STATE, "schedule not loaded");
    for (auto& kv : m->expected)
        if (!m->raw.count(kv.first)) return fail(DAD_E_KEY, "missing key '%s'", kv.first.c_str());
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(st));
    {
        const int rc0 = configure_kernels();
        if (rc0 != DAD_OK) return rc0;
    }
    free_device(m);
    const dad_cfg& c = m->cfg;
    if (m->training) if (const char* why = training_refusal(*m)) return fail(DAD_E_INVALID, "training: %s", why);
    m->weights = weight_table(*m);
    {
        void* a = nullptr;
        m->arena_cap = arena_bytes_needed(*m, m->weights);
        HIP_TRY(hipMalloc(&a, m->arena_cap));
        m->owned.push_back(a);
        m->arena = (char*)a;
        m->arena_used = 0;
    }

    HIP_TRY(hipGetDevice(&m->device));
    int rc;
    std::vector<float> host;
    for (WeightEntry& e : m->weights) {
        if ((rc = pack_entry(m, e, host)) != DAD_OK) return rc;
        if ((rc = upload(m, host, &e.dev)) != DAD_OK) return rc;
        weight_ptr(m, e) = e.dev;
    }
    for (size_t i = 0; i < m->plan.convs.size(); ++i) {        // the training plan launches the same images
        const ConvOp& a = m->plan.convs[i];
        ConvOp& b = m->tplan.convs[i];
        b.d_w = a.d_w; b.d_bias = a.d_bias; b.d_gamma = a.d_gamma; b.d_beta = a.d_beta; b.d_rbias = a.d_rbias;
        b.c1 = a.c1; b.c2 = a.c2;
    }
    if (m->training) {
        std::vector<float> zeros((size_t)std::max(m->max_bwd_m, 2 * m->max_cout) + 64, 0.0f);
        if ((rc = upload(m, zeros, &m->d_zero)) != DAD_OK) return rc;
        for (HostModel::BwdConv& b : m->bconvs)
            for (int k = 0; k < b.n; ++k) b.op[k].d_bias = m->d_zero;
        m->bfinal.d_bias = m->d_zero;
    }

    // ---- time-embedding tables: every t in [0, T) at once --------------------------------
    const int T = c.n_timesteps, dim = c.dim, tdm = c.time_dim;
    // SinusoidalPosEmb (temporal_unet.py:27-31): the caller's table when one was handed over
    // (dad_model_load_time_embedding: the Python mirror evaluates the reference's own torch
    // expression), else the same formula with the C library's expf/sinf/cosf
    const std::vector<float> emb = m->emb_override.size() == (size_t)T * dim ? m->emb_override
                                                                            : sinusoid_table(T, dim);
    float *d_emb, *d_h1, *d_temb;
    (void)c; (void)dim;
    if ((rc = upload(m, emb, &d_emb)) != DAD_OK) return rc;
    std::vector<float> zeros((size_t)T * 4 * tdm, 0.0f);
    if ((rc = upload(m, zeros, &d_h1)) != DAD_OK) return rc;
    zeros.resize((size_t)T * tdm);
    if ((rc = upload(m, zeros, &d_temb)) != DAD_OK) return rc;
    zeros.assign((size_t)T * std::max(1, m->plan.temb_width), 0.0f);
    if ((rc = upload(m, zeros, &m->d_temb_table)) != DAD_OK) return rc;
    m->d_emb = d_emb; m->d_temb = d_temb; m->d_h1 = d_h1;
    if ((rc = build_time_tables(m, st)) != DAD_OK) return rc;
    void* rng = nullptr;
    if ((rc = arena_alloc(m, 64, &rng)) != DAD_OK) return rc;
    m->d_rng = (uint64_t*)rng;
    void* cnt = nullptr;
    if ((rc = arena_alloc(m, kMaxSplitTiles * sizeof(unsigned), &cnt)) != DAD_OK) return rc;
    HIP_TRY(hipMemsetAsync(cnt, 0, kMaxSplitTiles * sizeof(unsigned), st));
    m->d_counters = (unsigned*)cnt;
    HIP_TRY(hipStreamSynchronize(st));
    if (!m->train_sched[0].empty() && (rc = upload_train_schedule(m)) != DAD_OK) return rc;
    m->raw.clear();
    m->finalized = true;
    return DAD_OK;
}

int dad_workspace_bytes(const dad_model* m, int32_t batch, size_t* bytes) {
    if (!m || !bytes || batch <= 0) return fail(DAD_E_INVALID, "bad argument");
    *bytes = workspace_bytes(*m, batch);
    return DAD_OK;
}

int dad_unet_forward(dad_model* m, const float* x, int32_t t, float* out, int32_t batch,
                     void* workspace, size_t workspace_bytes, dad_stream_t stream) {
    FwdPlan f;
    int rc = check_ready(m, batch, t, workspace_bytes, true, f);
    if (rc != DAD_OK) return rc;
    if (!x || !out || !workspace) return fail(DAD_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_tables(m, st)) != DAD_OK) return rc;
    if ((rc = run_unet(m, f, x, t, (float*)workspace, st)) != DAD_OK) return rc;
    return run_final(m, f, nullptr, x, t, nullptr, nullptr, 1, out, (float*)workspace, st);
}

int dad_unet_forward_rows(dad_model* m, const float* x, const int32_t* t_rows, float* out, int32_t batch,
                          void* workspace, size_t workspace_bytes, dad_stream_t stream) {
    FwdPlan f;
    int rc = check_ready(m, batch, 0, workspace_bytes, false, f);      // per-row timesteps: the batch kernels
    if (rc != DAD_OK) return rc;
    if (!x || !out || !workspace || !t_rows) return fail(DAD_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_tables(m, st)) != DAD_OK) return rc;
    if ((rc = run_unet(m, f, x, 0, (float*)workspace, st, t_rows)) != DAD_OK) return rc;
    return run_final(m, f, nullptr, x, 0, nullptr, nullptr, 1, out, (float*)workspace, st);
}

int dad_denoise_step(dad_model* m, float* x, int32_t t, int32_t batch, const dad_step_args* args,
                     int32_t x_out_disabled, void* workspace, size_t workspace_bytes,
                     dad_stream_t stream) {
    FwdPlan f;
    int rc = check_ready(m, batch, t, workspace_bytes, true, f);
    if (rc != DAD_OK) return rc;
    const dad_sampler_coef s = schedule_step(m, t);
    return sampler_step(m, f, x, s, args, x_out_disabled, workspace, stream);
}

int dad_sampler_step(dad_model* m, float* x, const dad_sampler_coef* coef, int32_t batch, const dad_step_args* args,
                     int32_t x_out_disabled, void* workspace, size_t workspace_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    int rc = check_sampler_steps(coef, 1, m->cfg.n_timesteps);
    if (rc != DAD_OK) return rc;
    FwdPlan f;
    if ((rc = check_ready(m, batch, coef->t, workspace_bytes, true, f)) != DAD_OK) return rc;
    return sampler_step(m, f, x, *coef, args, x_out_disabled, workspace, stream);
}

int dad_project(const dad_project_args* p, float alpha, float* x, int32_t batch, int32_t horizon,
                dad_stream_t stream) {
    if (!x || batch <= 0 || horizon <= 0) return fail(DAD_E_INVALID, "bad argument");
    return run_project(p, alpha, x, batch, horizon, (hipStream_t)stream);
}

int dad_projection_violation(const dad_project_args* p, const float* x, float* violation, int32_t batch,
                             int32_t horizon, dad_stream_t stream) {
    if (!x || !violation || batch <= 0 || horizon <= 0) return fail(DAD_E_INVALID, "bad argument");
    return run_project(p, 1.0f, const_cast<float*>(x), batch, horizon, (hipStream_t)stream, violation);
}

int dad_violation_grad_workspace_bytes(const dad_project_args* p, int32_t batch, int32_t horizon, int32_t form, size_t* bytes) {
    if (!p || !bytes) return fail(DAD_E_INVALID, "violation gradient: null pointer");
    int D = 0;
    ViolationGradPlan q;
    const int rc = violation_grad_plan_checked(p->state_dim, p->observation_dim, p->action_dim, batch, horizon, form, D, q);
    if (rc != DAD_OK) return rc;
    *bytes = q.workspace_bytes;
    return DAD_OK;
}

int dad_projection_violation_fwd(const dad_project_args* p, const float* x, float* violation, void* workspace,
                                 size_t workspace_bytes, int32_t batch, int32_t horizon, int32_t form, dad_stream_t stream) {
    return run_violation_fwd(p, x, violation, workspace, workspace_bytes, batch, horizon, form, (hipStream_t)stream);
}

int dad_projection_violation_bwd(const dad_project_args* p, const float* d_violation, float* d_x, void* workspace,
                                 size_t workspace_bytes, int32_t batch, int32_t horizon, int32_t form, dad_stream_t stream) {
    return run_violation_bwd(p, d_violation, d_x, workspace, workspace_bytes, batch, horizon, form, (hipStream_t)stream);
}

int dad_sample_loop(dad_model* m, float* x, int32_t n_steps, int32_t batch,
                    const float* noise_stack, uint64_t seed, uint64_t row_offset,
                    const float* cond0, int32_t cond_per_row, const dad_project_args* proj,
                    const float* proj_alphas_host, int32_t use_graph, void* workspace,
                    size_t workspace_bytes, dad_stream_t stream) {
    if (n_steps < 1) return fail(DAD_E_INVALID, "n_steps must be positive");
    FwdPlan f;                  // one description for all n_steps evaluations (and for a capture of them)
    int rc = check_ready(m, batch, n_steps - 1, workspace_bytes, true, f);
    if (rc != DAD_OK) return rc;
    if (proj && !proj_alphas_host) return fail(DAD_E_INVALID, "projection needs per-step alphas");
    // the ancestral sampler over the first n_steps entries of the loaded schedule, t = n_steps - 1 .. 0
    std::vector<dad_sampler_coef> steps((size_t)n_steps);
    std::vector<float> alphas(proj ? (size_t)n_steps : 0);
    for (int j = 0; j < n_steps; ++j) {
        steps[j] = schedule_step(m, n_steps - 1 - j);
        if (proj) alphas[j] = proj_alphas_host[n_steps - 1 - j];
    }
    return sampler_loop(m, f, x, steps.data(), n_steps, batch, noise_stack, seed, row_offset, cond0, cond_per_row, proj,
                        proj ? alphas.data() : nullptr, use_graph, workspace, stream);
}

int dad_sampler_loop(dad_model* m, float* x, const dad_sampler_coef* steps, int32_t n_steps, int32_t batch,
                     const float* noise_stack, uint64_t seed, uint64_t row_offset,
                     const float* cond0, int32_t cond_per_row, const dad_project_args* proj,
                     const float* proj_alphas_host, int32_t use_graph, void* workspace,
                     size_t workspace_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    int rc = check_sampler_steps(steps, n_steps, m->cfg.n_timesteps);
    if (rc != DAD_OK) return rc;
    FwdPlan f;
    if ((rc = check_ready(m, batch, steps[0].t, workspace_bytes, true, f)) != DAD_OK) return rc;
    return sampler_loop(m, f, x, steps, n_steps, batch, noise_stack, seed, row_offset, cond0, cond_per_row, proj,
                        proj_alphas_host, use_graph, workspace, stream);
}

int dad_guide_grad(const dad_guide_args* guide, const float* x, float* grad_out, float* value_rows_out, int32_t batch,
                   int32_t horizon, int32_t transition_dim, dad_stream_t stream) {
    GuideCall gc;
    int rc = guide_call_checked(guide, x, grad_out, value_rows_out, batch, horizon, transition_dim, gc);
    if (rc != DAD_OK || (rc = configure_kernels()) != DAD_OK) return rc;
    return launch_guide(gc, (hipStream_t)stream);
}

int dad_guided_loop(dad_model* m, float* x, const dad_sampler_coef* steps, int32_t n_steps, int32_t batch,
                    const float* noise_stack, uint64_t seed, uint64_t row_offset,
                    const float* cond0, int32_t cond_per_row, const dad_guide_args* guide, float guide_weight,
                    const dad_project_args* proj, const float* proj_alphas_host, int32_t use_graph, void* workspace,
                    size_t workspace_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (n_steps < 1) return fail(DAD_E_INVALID, "n_steps must be positive");
    std::vector<dad_sampler_coef> ancestral;
    int rc;
    if (steps != nullptr) {
        if ((rc = check_sampler_steps(steps, n_steps, m->cfg.n_timesteps)) != DAD_OK) return rc;
    }
    FwdPlan f;
    if ((rc = check_ready(m, batch, steps ? steps[0].t : n_steps - 1, workspace_bytes, true, f)) != DAD_OK) return rc;
    if (steps == nullptr) {                 // the ancestral sampler over the first n_steps entries of the loaded schedule
        ancestral.resize((size_t)n_steps);
        for (int j = 0; j < n_steps; ++j) ancestral[j] = schedule_step(m, n_steps - 1 - j);
        steps = ancestral.data();
    }
    return sampler_loop(m, f, x, steps, n_steps, batch, noise_stack, seed, row_offset, cond0, cond_per_row, proj,
                        proj_alphas_host, use_graph, workspace, stream, guide, guide_weight);
}

// ---------------------------------------------------------------------------------- training
int dad_model_set_training(dad_model* m, int32_t on) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (on) if (const char* why = training_refusal(*m)) return fail(DAD_E_INVALID, "training: %s", why);
    if ((on != 0) != m->training) m->finalized = false;       // the data-gradient images are packed at finalize
    m->training = on != 0;
    return DAD_OK;
}

int dad_model_refresh_weights(dad_model* m, int32_t n, const char* const* keys, const float* const* tensors,
                              dad_stream_t stream) {
    if (!m || n < 0 || (n > 0 && (!keys || !tensors))) return fail(DAD_E_INVALID, "bad argument");
    if (!m->finalized) return fail(DAD_E_STATE, "dad_model_finalize has not been called");
    if (m->precision != DAD_PREC_FP32)
        return fail(DAD_E_STATE, "the split-f16 images are scaled per layer on the host: load the weights and finalize again");
    hipStream_t st = (hipStream_t)stream;
    // A training loop refreshes after every optimiser step: the ~70 images and ~110 small tensors of a PointMaze
    // net were ~200 launches of ~5 us; they are collected here and go out as one repack launch (descriptor table in
    // device memory, re-uploaded only when a source address changed) and one copy launch per COPY_MAX tensors.
    std::vector<dad::ImageDesc> reps;
    std::vector<std::tuple<float*, const float*, size_t>> copies;
    std::map<std::string, const float*> given;
    for (int i = 0; i < n; ++i) {
        if (!keys[i] || !tensors[i]) return fail(DAD_E_INVALID, "null key or tensor at index %d", i);
        if (!m->expected.count(keys[i])) return fail(DAD_E_KEY, "unexpected key '%s'", keys[i]);
        given[keys[i]] = tensors[i];
    }
    auto has = [&](const std::string& k) -> const float* { auto it = given.find(k); return it == given.end() ? nullptr : it->second; };
    bool tables_dirty = false;
    for (const WeightEntry& e : m->weights) {
        const float* w = has(e.key);
        if (e.img.n == 0) {
            if (!w) continue;
            if ((size_t)e.floats >= (1u << 31)) return fail(DAD_E_INVALID, "refresh: a tensor of %zu floats", (size_t)e.floats);
            for (int r = 0; r < e.reps; ++r) copies.emplace_back(e.dev + r * e.floats, w, (size_t)e.floats);
            tables_dirty = tables_dirty || e.to == WT_TIME;
            continue;
        }
        // the image of a conv with a riding 1x1 residual conv holds both weights: both are needed to rebuild it
        const float* ride = e.key2.empty() ? nullptr : has(e.key2);
        if (!e.key2.empty() && (!w) != (!ride))
            return fail(DAD_E_KEY, "'%s' and '%s' share one packed image: refresh them together", e.key.c_str(), e.key2.c_str());
        if (!w) continue;
        dad::ImageDesc p = e.img;
        p.dst = e.dev; p.w = w; p.ride = ride;
        reps.push_back(p);
    }
    for (size_t at = 0; at < copies.size(); at += dad::COPY_MAX) {
        dad::CopyMany cm{};
        const int k = (int)std::min<size_t>(dad::COPY_MAX, copies.size() - at);
        size_t widest = 1;
        for (int i = 0; i < k; ++i) {
            cm.dst[i] = std::get<0>(copies[at + i]); cm.src[i] = std::get<1>(copies[at + i]);
            cm.n[i] = (int32_t)std::get<2>(copies[at + i]);
            widest = std::max(widest, std::get<2>(copies[at + i]));
        }
        const unsigned gx = (unsigned)std::min<size_t>(64, (widest + 1023) / 1024);
        hipLaunchKernelGGL(dad::copy_many_kernel, dim3(gx, (unsigned)k), dim3(256), 0, st, cm);
        HIP_TRY(hipGetLastError());
    }
    if (!reps.empty()) {
        std::vector<int> first(reps.size() + 1, 0);
        for (size_t i = 0; i < reps.size(); ++i) {
            const long blocks = (reps[i].n + 255) / 256;
            if (first[i] + blocks >= (1L << 31)) return fail(DAD_E_INVALID, "refresh: too many image elements for one launch");
            first[i + 1] = first[i] + (int)blocks;
        }
        const size_t desc_bytes = reps.size() * sizeof(dad::ImageDesc), first_bytes = first.size() * sizeof(int);
        const bool same = m->repack_host.size() == desc_bytes && std::memcmp(m->repack_host.data(), reps.data(), desc_bytes) == 0;
        if (!same) {
            if (m->repack_cap < desc_bytes + first_bytes) {       // (grows once; freed with the model's other allocations)
                void* a = nullptr;
                HIP_TRY(hipMalloc(&a, desc_bytes + first_bytes));
                m->owned.push_back(a);
                m->d_repack = a; m->repack_cap = desc_bytes + first_bytes;
            }
            HIP_TRY(hipStreamSynchronize(st));                    // a previous refresh may still read the table
            HIP_TRY(hipMemcpy(m->d_repack, reps.data(), desc_bytes, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy((char*)m->d_repack + desc_bytes, first.data(), first_bytes, hipMemcpyHostToDevice));
            m->repack_host.assign((const char*)reps.data(), (const char*)reps.data() + desc_bytes);
        }
        hipLaunchKernelGGL(dad::repack_many_kernel, dim3((unsigned)first.back()), dim3(256), 0, st,
                           (const dad::ImageDesc*)m->d_repack, (const int*)((const char*)m->d_repack + desc_bytes), (int)reps.size());
        HIP_TRY(hipGetLastError());
    }
    // the per-timestep tables belong to the sampler: a training loop never reads them, so they are re-derived by the
    // next inference entry point (ensure_tables), not after every optimiser step (14 launches, 0.35 ms on PointMaze)
    if (tables_dirty) m->tables_stale = true;
    return DAD_OK;
}

int dad_train_grad_count(const dad_model* m, int32_t* count, int64_t* total_floats) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (count) *count = (int32_t)m->grad_slots.size();
    if (total_floats) *total_floats = m->grad_numel;
    return DAD_OK;
}

int dad_train_grad_info(const dad_model* m, int32_t i, const char** key, int64_t* offset, int64_t* numel) {
    if (!m || i < 0 || i >= (int32_t)m->grad_slots.size()) return fail(DAD_E_INVALID, "gradient slot %d out of range", i);
    if (key) *key = m->grad_slots[i].key.c_str();
    if (offset) *offset = m->grad_slots[i].offset;
    if (numel) *numel = m->grad_slots[i].numel;
    return DAD_OK;
}

}  // extern "C"  (helpers of the training entry points follow)

namespace {

// weight-gradient step `s` of the backward plan, geometry `w` (train_scratch); split batches go through `wslab`
int launch_wgrad(const dad_model* m, const BwdStep& s, const TrainScratch::Wgrad& w, const float* G, const float* Z0,
                 const float* Z1, float* out, float* wslab, hipStream_t st) {
    const WgradGeom& g = w.g;
    dad::WgradParams p{};
    p.G = G; p.ldg = s.M; p.M = s.M;                    // ld == width everywhere
    p.Z0 = Z0; p.ldz0 = s.C0; p.C0 = s.C0; p.Z1 = Z1; p.ldz1 = s.C1; p.C1 = s.C1;
    p.out_numel = (long)s.M * (s.C0 + s.C1) * s.taps;
    p.out = g.ksplit > 1 ? wslab : out;
    p.B = w.sh.B; p.Lg = w.sh.Lg; p.Lz = w.sh.Lz; p.lg_shift = ilog2(w.sh.Lg); p.stride = s.stride; p.pad = s.pad;
    p.wshift = w.sh.wshift;
    p.ksplit = g.ksplit; p.samples_per_split = g.sps; p.spc = g.spc;
    p.zero = m->d_zero;
    const void* fn = find_kernel(FAM_WGRAD, {s.taps, g.tile, w.sh.wshift > 0});
    if (fn == nullptr) return fail(DAD_E_INVALID, "no weight-gradient kernel for %d taps on tile %d (windowed=%d)", s.taps, g.tile, (int)(w.sh.wshift > 0));
    void* args[] = {&p};
    HIP_TRY(hipLaunchKernel(fn, dim3(g.gx, g.gy, (unsigned)g.ksplit), dim3(dad::WG_THREADS), args, g.lds, st));
    if (g.ksplit > 1) {
        const long n4 = p.out_numel / 4;
        hipLaunchKernelGGL(dad::sum_slabs_kernel, dim3((unsigned)((n4 + 63) / 64)), dim3(256), 0, st, out, wslab, n4, g.ksplit);
        HIP_TRY(hipGetLastError());
    }
    return DAD_OK;
}

// y += x over n floats (n a multiple of 4), or y = x (BW_SET)
int accumulate(float* y, const float* x, long n, BwdWrite how, hipStream_t st) {
    if (how == BW_SET) { HIP_TRY(hipMemcpyAsync(y, x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st)); return DAD_OK; }
    const long n4 = n / 4;
    hipLaunchKernelGGL(dad::add_inplace_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, y, x, n4);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

int check_train(const dad_model* m, int batch) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!m->training) return fail(DAD_E_STATE, "dad_model_set_training(m, 1) has not been called");
    if (!m->finalized) return fail(DAD_E_STATE, "dad_model_finalize has not been called");
    if (batch <= 0) return fail(DAD_E_INVALID, "batch must be positive (got %d)", batch);
    return DAD_OK;
}

}  // namespace

extern "C" {

int dad_train_workspace_bytes(const dad_model* m, int32_t batch, size_t* saved_bytes, size_t* scratch_bytes) {
    if (!m || batch <= 0) return fail(DAD_E_INVALID, "bad argument");
    if (saved_bytes) {
        FwdPlan f;
        plan_forward(*m, true, batch, false, f);       // (as below: a refused batch still has a size)
        *saved_bytes = f.bytes;
    }
    if (scratch_bytes) {
        TrainScratch ts;
        train_scratch(*m, batch, ts);          // a batch the backward pass refuses is refused there, not here
        *scratch_bytes = (size_t)ts.total * sizeof(float);
    }
    return DAD_OK;
}

int dad_unet_forward_train(dad_model* m, const float* x, const int32_t* row_index, const float* temb_rows,
                           float* out, int32_t batch, void* saved, size_t saved_bytes, dad_stream_t stream) {
    int rc = check_train(m, batch);
    if (rc != DAD_OK) return rc;
    if (!x || !row_index || !temb_rows || !out || !saved) return fail(DAD_E_INVALID, "null pointer");
    FwdPlan f;
    rc = plan_forward(*m, true, batch, false, f);
    if (saved_bytes < f.bytes)
        return fail(DAD_E_WORKSPACE, "saved-activation buffer has %zu bytes, batch %d needs %zu", saved_bytes, batch, f.bytes);
    if (rc != DAD_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_unet(m, f, x, 0, (float*)saved, st, row_index, temb_rows)) != DAD_OK) return rc;
    return run_final(m, f, nullptr, x, 0, nullptr, nullptr, 1, out, (float*)saved, st);
}

// `pre`: the pass as the fused objective already planned it for this batch (nothing is planned twice per call);
// `before_launch`: what the fused objective enqueues behind every refusal of the pass and ahead of its first launch
static int unet_backward(dad_model* m, const float* x, const float* d_out, float* d_x, float* d_temb_rows,
                         float* const* grad_tensors, int32_t n_grad_tensors,
                         int32_t batch, void* saved_v, size_t saved_bytes, void* scratch_v, size_t scratch_bytes,
                         dad_stream_t stream, const ObjectivePlan* pre = nullptr,
                         const std::function<int()>* before_launch = nullptr) {
    int rc = check_train(m, batch);
    if (rc != DAD_OK) return rc;
    if (!x || !d_out || !d_temb_rows || !grad_tensors || !saved_v || !scratch_v) return fail(DAD_E_INVALID, "null pointer");
    if (n_grad_tensors != (int32_t)m->grad_slots.size())
        return fail(DAD_E_INVALID, "%d gradient tensors passed, the model has %zu (dad_train_grad_count)", n_grad_tensors,
                    m->grad_slots.size());
    for (int32_t i = 0; i < n_grad_tensors; ++i)
        if (!grad_tensors[i]) return fail(DAD_E_INVALID, "gradient tensor %d ('%s') is null", i, m->grad_slots[i].key.c_str());
    const int B = batch;
    FwdPlan fwd_own;                               // (read for the size of `saved` alone)
    TrainScratch ts_own;
    int geom_rc = DAD_OK;                          // (a pre-planned pass was refused where it was planned)
    if (pre == nullptr) {
        plan_forward(*m, true, B, false, fwd_own);
        geom_rc = train_scratch(*m, B, ts_own);
    }
    const size_t fwd_bytes = pre ? pre->fwd.bytes : fwd_own.bytes;
    const TrainScratch& ts = pre ? pre->ts : ts_own;
    if (saved_bytes < fwd_bytes || scratch_bytes < (size_t)ts.total * sizeof(float))
        return fail(DAD_E_WORKSPACE, "backward workspaces too small (saved %zu / %zu, scratch %zu / %zu bytes)", saved_bytes,
                    fwd_bytes, scratch_bytes, (size_t)ts.total * sizeof(float));
    if (m->bwd_rc != DAD_OK) return fail(m->bwd_rc, "%s", m->bwd_err.c_str());
    if (geom_rc != DAD_OK) return geom_rc;
    if (d_x != nullptr && !m->bdx) return fail(DAD_E_STATE, "backward: no gradient reached the trajectory");
    if (before_launch != nullptr && (rc = (*before_launch)()) != DAD_OK) return rc;

    hipStream_t st = (hipStream_t)stream;
    const Plan& P = m->tplan;
    const int H = m->cfg.horizon, td = m->cfg.transition_dim, tdp = round_up(td, 32);
    float* const saved = (float*)saved_v;
    float* const mirror = (float*)scratch_v;
    float* const part = mirror + ts.mirror;
    float* const wslab = part + ts.part;
    float* const dxpad = wslab + ts.wslab;
    float* const tmp = dxpad + ts.dxpad;
    float* const bslab = tmp + ts.tmp;
    // zero-padded horizon: the trajectory and d loss / d out arrive in their real shape (B, H_real, td); the pass runs on
    // copies in the padded layout (zero rows behind the real ones), d x goes back through the same row map
    const int Hr = traj_horizon(*m);
    if (Hr != H) {
        float* const xpad = dxpad + (long)B * H * tdp;
        float* const dopad = xpad + (long)B * H * round_up(td, 4);
        const long n = (long)B * H * td;
        hipLaunchKernelGGL(dad::pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, xpad, x, (long)B, H, Hr, td);
        hipLaunchKernelGGL(dad::pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dopad, d_out, (long)B, H, Hr, td);
        HIP_TRY(hipGetLastError());
        x = xpad; d_out = dopad;
    }
    auto ptr = [&](const BwdRef& r) -> float* {
        switch (r.sp) {
            case BSP_ACT: return saved + P.bufs[r.buf].offset * (long)B;
            case BSP_GRAD: return mirror + P.bufs[r.buf].offset * (long)B;
            case BSP_X: return const_cast<float*>(x);                 // read only
            case BSP_DOUT: return const_cast<float*>(d_out);          // read only
            case BSP_DX: return dxpad;
            default: return nullptr;
        }
    };

    // the steps of the backward plan (build_backward_plan), in order
    size_t nw = 0, nd = 0;
    for (const BwdStep& s : m->bsteps) {
        switch (s.kind) {
            case BK_BIAS:
                hipLaunchKernelGGL(dad::row_partial_sums_kernel, dim3(B), dim3(256), 0, st, part + s.part * B, ptr(s.in),
                                   s.rows, s.C, s.C);
                HIP_TRY(hipGetLastError());
                break;
            case BK_WGRAD:
                if ((rc = launch_wgrad(m, s, ts.wgrads[nw++], ptr(s.in), ptr(s.z0), ptr(s.z1), grad_tensors[s.slot], wslab, st)) != DAD_OK)
                    return rc;
                break;
            case BK_DGRAD: {
                ConvIO io;
                io.src0 = ptr(s.in); io.slab = bslab;
                io.dst = s.write == BW_STAGE ? tmp : ptr(s.out);
                io.res = s.write == BW_ADD ? io.dst : nullptr;
                if ((rc = launch_conv(m, bwd_op(*m, s), ts.dgrads[nd++].g, B, io, st)) != DAD_OK) return rc;
                if (s.write == BW_STAGE && (rc = accumulate(ptr(s.out), tmp, s.n * B, BW_ADD, st)) != DAD_OK) return rc;
                break;
            }
            case BK_GN: {
                const ConvOp& f = P.convs[s.conv];
                const long c4 = round_up(f.cout, 4);
                dad::GnBwdParams gp{};
                gp.dA = ptr(s.in); gp.h = saved + P.bufs[f.pre].offset * (long)B; gp.stats = saved + P.bufs[f.stats].offset * (long)B;
                gp.gamma = f.d_gamma; gp.beta = f.d_beta;
                gp.dH = ptr(s.out);
                gp.part_dgamma = part + s.part * B; gp.part_dbeta = gp.part_dgamma + c4 * B; gp.part_dbias = gp.part_dbeta + c4 * B;
                const GnBwdShape q = gn_bwd_shape(f);
                gp.dtemb = q.dtemb ? d_temb_rows + f.temb_off : nullptr;
                gp.temb_stride = P.temb_width;
                gp.C = q.C; gp.L = q.L; gp.cpg = q.cpg; gp.lreal = q.lreal; gp.cpg_real = q.cpg_real;
                gp.B = B;
                const dim3 wgrid((unsigned)((B * 8 + 3) / 4));
                switch (s.nv) {
                    case 1: hipLaunchKernelGGL(dad::gn_mish_bwd_wave_kernel<1>, wgrid, dim3(256), 0, st, gp); break;
                    case 2: hipLaunchKernelGGL(dad::gn_mish_bwd_wave_kernel<2>, wgrid, dim3(256), 0, st, gp); break;
                    case 4: hipLaunchKernelGGL(dad::gn_mish_bwd_wave_kernel<4>, wgrid, dim3(256), 0, st, gp); break;
                    case 8: hipLaunchKernelGGL(dad::gn_mish_bwd_wave_kernel<8>, wgrid, dim3(256), 0, st, gp); break;
                    case 16: hipLaunchKernelGGL(dad::gn_mish_bwd_wave_kernel<16>, wgrid, dim3(256), 0, st, gp); break;
                    default: hipLaunchKernelGGL(dad::gn_mish_bwd_kernel, dim3(B, 8), dim3(dad::GNB_THREADS), 0, st, gp);
                }
                HIP_TRY(hipGetLastError());
                break;
            }
            case BK_RESID:
                if ((rc = accumulate(ptr(s.out), ptr(s.in), s.n * B, s.write, st)) != DAD_OK) return rc;
                break;
            case BK_COLS: {
                const long rows = (long)B * s.rows, n4 = rows * (s.C / 4);
                hipLaunchKernelGGL(dad::take_cols_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                                   ptr(s.out), ptr(s.in), rows, s.C, s.ld, s.off, (int)(s.write == BW_ADD));
                HIP_TRY(hipGetLastError());
                break;
            }
        }
    }
    // every layer's per-sample partial sums, reduced over the batch by as few launches as the argument block allows
    for (size_t at = 0; at < m->bsums.size(); at += dad::COLS_MAX) {
        dad::ColSumsMany cs{};
        const int n = (int)std::min<size_t>(dad::COLS_MAX, m->bsums.size() - at);
        int widest = 0;
        for (int k = 0; k < n; ++k) {
            const BwdSum& q = m->bsums[at + k];
            cs.out[k] = grad_tensors[q.slot]; cs.part[k] = part + q.part * B; cs.C[k] = q.C;
            widest = std::max(widest, q.C);
        }
        hipLaunchKernelGGL(dad::col_sums_many_kernel, dim3((unsigned)((widest + 31) / 32), (unsigned)n), dim3(256), 0, st, cs, B);
        HIP_TRY(hipGetLastError());
    }
    if (d_x != nullptr) {
        const long n = (long)B * Hr * td;
        if (Hr != H)
            hipLaunchKernelGGL(dad::slice_rows_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_x, dxpad, (long)B, H, Hr, td, tdp);
        else
            hipLaunchKernelGGL(dad::slice_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_x, dxpad, (long)B * H, td, tdp);
        HIP_TRY(hipGetLastError());
    }
    return DAD_OK;
}

int dad_unet_backward(dad_model* m, const float* x, const float* d_out, float* d_x, float* d_temb_rows,
                      float* const* grad_tensors, int32_t n_grad_tensors,
                      int32_t batch, void* saved_v, size_t saved_bytes, void* scratch_v, size_t scratch_bytes,
                      dad_stream_t stream) {
    return unet_backward(m, x, d_out, d_x, d_temb_rows, grad_tensors, n_grad_tensors, batch, saved_v, saved_bytes, scratch_v,
                         scratch_bytes, stream);
}

// ------------------------------------------------------------------------- fused training objective
int dad_train_time_grad_count(const dad_model* m, int32_t* count, int64_t* total_floats) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (count) *count = (int32_t)m->time_grad_slots.size();
    if (total_floats) *total_floats = m->time_grad_numel;
    return DAD_OK;
}

int dad_train_time_grad_info(const dad_model* m, int32_t i, const char** key, int64_t* offset, int64_t* numel) {
    if (!m || i < 0 || i >= (int32_t)m->time_grad_slots.size()) return fail(DAD_E_INVALID, "time gradient slot %d out of range", i);
    if (key) *key = m->time_grad_slots[i].key.c_str();
    if (offset) *offset = m->time_grad_slots[i].offset;
    if (numel) *numel = m->time_grad_slots[i].numel;
    return DAD_OK;
}

int dad_train_objective_workspace_bytes(const dad_model* m, int32_t batch, size_t* saved_bytes, size_t* scratch_bytes) {
    if (!m || batch <= 0) return fail(DAD_E_INVALID, "bad argument");
    ObjectiveLayout o;
    objective_layout(*m, batch, o);        // (as dad_train_workspace_bytes: a refused batch still has a size)
    if (saved_bytes) *saved_bytes = o.saved_bytes;
    if (scratch_bytes) *scratch_bytes = o.scratch_bytes;
    return DAD_OK;
}

int dad_debug_objective_offsets(const dad_model* m, int32_t batch, size_t* xt_offset, size_t* out_offset) {
    if (!m || batch <= 0) return fail(DAD_E_INVALID, "bad argument");
    ObjectiveLayout o;
    objective_layout(*m, batch, o);
    if (xt_offset) *xt_offset = o.saved_base + (size_t)o.xt * sizeof(float);
    if (out_offset) *out_offset = o.saved_base + (size_t)o.out * sizeof(float);
    return DAD_OK;
}

}  // extern "C"  (helpers of the objective entry points follow)

namespace {

// Every refusal the two objective entry points share, in the order the header documents; `plan`: everything of the
// call that is planned on the host, once (`backward`: with the backward pass's geometry)
int check_objective(const dad_model* m, int batch, int loss_type, bool backward, ObjectivePlan& plan) {
    if (loss_type != DAD_LOSS_L1 && loss_type != DAD_LOSS_L2)
        return fail(DAD_E_INVALID, "unknown loss_type %d (DAD_LOSS_L1 = 1, DAD_LOSS_L2 = 2)", loss_type);
    if (!m->training) return fail(DAD_E_INVALID, "training mode is off: dad_model_set_training(m, 1) before dad_model_finalize");
    if (m->precision != DAD_PREC_FP32) return fail(DAD_E_INVALID, "the training objective exists for the fp32 arithmetic only, not split-f16");
    if (batch <= 0) return fail(DAD_E_INVALID, "batch must be positive (got %d)", batch);
    if (!m->finalized) return fail(DAD_E_STATE, "dad_model_finalize has not been called");
    if (m->d_train_sched == nullptr) return fail(DAD_E_STATE, "dad_model_load_train_schedule has not been called");
    return objective_plan(*m, batch, backward, plan);
}

const float* time_tensor(const dad_model* m, const std::string& key) {
    const auto it = m->d_time.find(key);
    return it == m->d_time.end() ? nullptr : it->second;
}

// the blocks' time_mlp.1 tensors (device copies: what dad_model_refresh_weights keeps current) and, backward, their
// gradient tensors (`tg`: the time gradient list, blocks from entry 4 on)
int fill_time_blocks(const dad_model* m, dad::TimeBlocks& tb, float* const* tg) {
    const std::vector<TimeBlockRef> list = time_block_list(*m);
    tb = dad::TimeBlocks{};
    tb.n = (int32_t)list.size();
    for (size_t k = 0; k < list.size(); ++k) {
        tb.w[k] = time_tensor(m, list[k].base + ".time_mlp.1.weight");
        tb.b[k] = time_tensor(m, list[k].base + ".time_mlp.1.bias");
        if (!tb.w[k] || !tb.b[k]) return fail(DAD_E_KEY, "missing key '%s.time_mlp.1'", list[k].base.c_str());
        tb.off[k] = list[k].off;
        if (tg != nullptr) { tb.dw[k] = tg[4 + 2 * k]; tb.db[k] = tg[5 + 2 * k]; }
    }
    tb.off[list.size()] = m->tplan.temb_width;
    return DAD_OK;
}

static_assert(dad::TG_FWD_H1 == DAD_OP_TG_FWD_H1 && dad::TG_FWD_TEMB == DAD_OP_TG_FWD_TEMB && dad::TG_FWD_ROWS == DAD_OP_TG_FWD_ROWS &&
              dad::TG_BWD_DWK == DAD_OP_TG_BWD_DWK && dad::TG_BWD_DACT == DAD_OP_TG_BWD_DACT && dad::TG_BWD_DW3 == DAD_OP_TG_BWD_DW3 &&
              dad::TG_BWD_DH1 == DAD_OP_TG_BWD_DH1 && dad::TG_BWD_DW1 == DAD_OP_TG_BWD_DW1, "DAD_OP_TG_* name the TimeGemm modes");

// Launch `l` of the planned time chain (ObjectivePlan::time): its geometry is the list's, the operands are `p`'s
template <int MODE>
int launch_time_gemm(dad::TimeGemmParams& p, const TimeLaunch& l, hipStream_t st) {
    if (l.mode != MODE) return fail(DAD_E_STATE, "time chain: launch %d planned where %d runs", l.mode, MODE);
    p.M = l.M; p.N = l.N; p.K = l.K; p.kslice = l.kslice;
    hipLaunchKernelGGL(dad::time_gemm_kernel<MODE>, dim3(l.gx(), l.gy(), l.gz()), dim3(dad::TG_THREADS), 0, st, p);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

dad::ObjectiveParams objective_params(const dad_model* m, const ObjectiveLayout& o, float* sv, int batch, int loss_type,
                                      const float* x0, const float* noise, const float* weights) {
    dad::ObjectiveParams q{};
    const int T = m->cfg.n_timesteps;
    q.x0 = x0; q.noise = noise; q.weights = weights;
    q.sqrt_ac = m->d_train_sched; q.sqrt_1m_ac = m->d_train_sched + T;
    q.t_rows = (int32_t*)(sv + o.t_rows); q.row_index = (int32_t*)(sv + o.row_index);
    q.xt = sv + o.xt; q.out = sv + o.out; q.partial = sv + o.partial;
    q.row_elems = traj_horizon(*m) * m->cfg.transition_dim;
    q.n = (long)batch * q.row_elems;
    q.B = batch; q.T = T;
    q.l1 = loss_type == DAD_LOSS_L1;
    q.predict_epsilon = m->cfg.predict_epsilon;
    q.nblocks = o.loss_blocks;
    return q;
}

// How every plan report leaves: its length in *needed_out, min(capacity, length) ints in `out`.
int copy_report(const std::vector<int32_t>& r, int32_t* out, int32_t capacity, int32_t* needed_out) {
    if (needed_out) *needed_out = (int32_t)r.size();
    std::copy(r.begin(), r.begin() + std::min<size_t>(r.size(), (size_t)capacity), out);
    return DAD_OK;
}
// A report of the training step: needs a backward plan; a batch the pass (or the objective) refuses is refused here too.
int training_report(const dad_model* m, int32_t batch, int (*report)(const HostModel&, int, std::vector<int32_t>&), int32_t* out,
                    int32_t capacity, int32_t* needed_out) {
    if (!m || batch <= 0 || capacity < 0 || (capacity > 0 && !out)) return fail(DAD_E_INVALID, "bad argument");
    if (!m->training) return fail(DAD_E_STATE, "dad_model_set_training(m, 1) has not been called");
    if (m->bwd_rc != DAD_OK) return fail(m->bwd_rc, "%s", m->bwd_err.c_str());
    std::vector<int32_t> r;
    const int rc = report(*m, batch, r);
    return rc != DAD_OK ? rc : copy_report(r, out, capacity, needed_out);
}

// The forward of the fused objective once it is planned and its arguments are checked: everything
// dad_train_objective_forward launches (the dynamics-aware objective runs the same launches first).
int objective_forward_run(dad_model* m, const ObjectivePlan& plan, const float* x0, const int32_t* t_rows, const float* noise,
                          const float* weights, int32_t loss_type, float* loss_out, int32_t batch, void* saved, dad_stream_t stream) {
    int rc = DAD_OK;
    const ObjectiveLayout& o = plan.o;
    const FwdPlan& f = plan.fwd;
    const dad_cfg& c = m->cfg;
    const int tdm = c.time_dim;
    const std::vector<TimeLaunch>& tl = plan.time;        // [0, 3): the forward's
    const float *w1 = time_tensor(m, "time_mlp.1.weight"), *b1 = time_tensor(m, "time_mlp.1.bias");
    const float *w3 = time_tensor(m, "time_mlp.3.weight"), *b3 = time_tensor(m, "time_mlp.3.bias");
    if (!w1 || !b1 || !w3 || !b3) return fail(DAD_E_KEY, "missing key 'time_mlp'");
    dad::TimeGemmParams g{};
    if ((rc = fill_time_blocks(m, g.tb, nullptr)) != DAD_OK) return rc;

    hipStream_t st = (hipStream_t)stream;
    float* const sv = (float*)((char*)saved + o.saved_base);
    dad::ObjectiveParams q = objective_params(m, o, sv, batch, loss_type, x0, noise, weights);
    q.t_in = t_rows; q.loss = loss_out;
    // 1. x_t = q_sample(x_0, t, noise); clamped timesteps and the row index of the projections (diffusion.py:138-157)
    hipLaunchKernelGGL(dad::objective_xt_kernel, dim3((unsigned)((std::max<long>(q.n, batch) + 255) / 256)), dim3(dad::OBJ_THREADS), 0, st, q);
    HIP_TRY(hipGetLastError());
    // 2. the time chain per row (temporal_unet.py:19-32,155-160 and every block's :97-100)
    g.emb = m->d_emb; g.t_rows = q.t_rows;
    g.w = w1; g.ldw = c.dim; g.bias = b1; g.out = sv + o.h1;
    if ((rc = launch_time_gemm<dad::TG_FWD_H1>(g, tl[0], st)) != DAD_OK) return rc;
    g.a = sv + o.h1; g.lda = 4 * tdm; g.w = w3; g.ldw = 4 * tdm; g.bias = b3; g.out = sv + o.temb; g.out2 = sv + o.act;
    if ((rc = launch_time_gemm<dad::TG_FWD_TEMB>(g, tl[1], st)) != DAD_OK) return rc;
    g.a = sv + o.act; g.lda = tdm; g.out = sv + o.rows; g.out2 = nullptr;
    if ((rc = launch_time_gemm<dad::TG_FWD_ROWS>(g, tl[2], st)) != DAD_OK) return rc;
    // the denoiser's training forward on x_t (diffusion.py:272), every activation kept
    if ((rc = run_unet(m, f, q.xt, 0, (float*)saved, st, q.row_index, sv + o.rows)) != DAD_OK) return rc;
    if ((rc = run_final(m, f, nullptr, q.xt, 0, nullptr, nullptr, 1, sv + o.out, (float*)saved, st)) != DAD_OK) return rc;
    // 3. weighted L1 / L2 mean (diffusion.py:274-290)
    hipLaunchKernelGGL(dad::objective_loss_partial_kernel, dim3((unsigned)q.nblocks), dim3(dad::OBJ_THREADS), 0, st, q);
    hipLaunchKernelGGL(dad::objective_loss_final_kernel, dim3(1), dim3(dad::OBJ_THREADS), 0, st, q);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

// The backward of the fused objective once it is planned: the rest of dad_train_objective_backward's refusals, then
// its launches.  `need_saved` / `need_scratch`: what the caller's buffers must hold.  `head`: what writes d loss / d out
// (enqueued behind every refusal of the denoiser's pass, ahead of its first launch) when it is not objective_dout_kernel.
int objective_backward_run(dad_model* m, const ObjectivePlan& plan, const float* x0, const float* noise, const float* weights,
                           int32_t loss_type, const float* d_loss, float* const* grad_tensors, int32_t n_grad_tensors,
                           float* const* time_grad_tensors, int32_t n_time_grad_tensors, int32_t batch, void* saved,
                           size_t saved_bytes, size_t need_saved, void* scratch, size_t scratch_bytes, size_t need_scratch,
                           dad_stream_t stream, const std::function<int(const dad::ObjectiveParams&)>* head_of) {
    int rc = DAD_OK;
    const ObjectiveLayout& o = plan.o;
    // (both counts before either list is walked)
    if (n_grad_tensors != (int32_t)m->grad_slots.size())
        return fail(DAD_E_INVALID, "%d gradient tensors passed, the model has %zu (dad_train_grad_count)", n_grad_tensors, m->grad_slots.size());
    if (n_time_grad_tensors != (int32_t)m->time_grad_slots.size())
        return fail(DAD_E_INVALID, "%d time gradient tensors passed, the model has %zu (dad_train_time_grad_count)", n_time_grad_tensors,
                    m->time_grad_slots.size());
    for (int32_t i = 0; i < n_time_grad_tensors; ++i)
        if (!time_grad_tensors[i]) return fail(DAD_E_INVALID, "time gradient tensor %d ('%s') is null", i, m->time_grad_slots[i].key.c_str());
    if (saved_bytes < need_saved || scratch_bytes < need_scratch)
        return fail(DAD_E_WORKSPACE, "objective workspaces too small (saved %zu / %zu, scratch %zu / %zu bytes)", saved_bytes, need_saved,
                    scratch_bytes, need_scratch);
    float* const sv = (float*)((char*)saved + o.saved_base);
    float* const sc = (float*)((char*)scratch + o.scratch_base);
    const int tdm = m->cfg.time_dim, W = m->tplan.temb_width;
    const std::vector<TimeLaunch>& tl = plan.time;        // [3, 9): the backward's
    const float* w3 = time_tensor(m, "time_mlp.3.weight");
    if (!w3) return fail(DAD_E_KEY, "missing key 'time_mlp.3.weight'");
    dad::TimeGemmParams g{};
    if ((rc = fill_time_blocks(m, g.tb, time_grad_tensors)) != DAD_OK) return rc;

    hipStream_t st = (hipStream_t)stream;
    dad::ObjectiveParams q = objective_params(m, o, sv, batch, loss_type, x0, noise, weights);
    q.d_loss = d_loss; q.d_out = sc + o.d_out;
    // d loss / d out, scaled by autograd's incoming scalar on the device: enqueued by the denoiser's pass behind its own
    // refusals, ahead of its first launch
    const std::function<int()> head = [&]() -> int {
        if (head_of != nullptr) return (*head_of)(q);
        hipLaunchKernelGGL(dad::objective_dout_kernel, dim3((unsigned)((q.n + 255) / 256)), dim3(dad::OBJ_THREADS), 0, st, q);
        HIP_TRY(hipGetLastError());
        return DAD_OK;
    };
    if ((rc = unet_backward(m, sv + o.xt, sc + o.d_out, nullptr, sc + o.d_rows, grad_tensors, n_grad_tensors, batch, saved, saved_bytes,
                            scratch, scratch_bytes, stream, &plan, &head)) != DAD_OK) return rc;
    // 4. the time chain backwards: six launches
    g.emb = m->d_emb; g.t_rows = q.t_rows;
    g.a = sc + o.d_rows; g.lda = W; g.w = sv + o.act; g.ldw = tdm;         // d Wk = d rows^T act, d bk
    if ((rc = launch_time_gemm<dad::TG_BWD_DWK>(g, tl[3], st)) != DAD_OK) return rc;
    g.out = sc + o.dact_slab;                                              // d act = d rows W, K slices in slabs
    if ((rc = launch_time_gemm<dad::TG_BWD_DACT>(g, tl[4], st)) != DAD_OK) return rc;
    {
        const TimeLaunch& l = tl[5];
        if (l.mode != DAD_OP_TG_DTEMB) return fail(DAD_E_STATE, "time chain: launch %d planned where the slab sum runs", l.mode);
        hipLaunchKernelGGL(dad::time_dtemb_kernel, dim3(l.gx(), l.gy(), l.gz()), dim3(256), 0, st, sc + o.dtemb,
                           sc + o.dact_slab, sv + o.temb, (long)l.M * l.N, l.K);
        HIP_TRY(hipGetLastError());
    }
    g.a = sc + o.dtemb; g.lda = tdm; g.w = sv + o.h1; g.ldw = 4 * tdm; g.out = time_grad_tensors[2]; g.out2 = time_grad_tensors[3];
    if ((rc = launch_time_gemm<dad::TG_BWD_DW3>(g, tl[6], st)) != DAD_OK) return rc;        // d W3 = d temb^T mish(h1), d b3
    g.w = w3; g.ldw = 4 * tdm; g.h1 = sv + o.h1; g.out = sc + o.dh1; g.out2 = nullptr;      // d h1 = (d temb W3) mish'(h1)
    if ((rc = launch_time_gemm<dad::TG_BWD_DH1>(g, tl[7], st)) != DAD_OK) return rc;
    g.a = sc + o.dh1; g.lda = 4 * tdm; g.out = time_grad_tensors[0]; g.out2 = time_grad_tensors[1];
    return launch_time_gemm<dad::TG_BWD_DW1>(g, tl[8], st);                                 // d W1 = d h1^T emb, d b1
}

}  // namespace

extern "C" {

int dad_train_objective_forward(dad_model* m, const float* x0, const int32_t* t_rows, const float* noise,
                                const float* weights, int32_t loss_type, float* loss_out, int32_t batch, void* saved,
                                size_t saved_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!x0 || !t_rows || !noise || !loss_out || !saved) return fail(DAD_E_INVALID, "null pointer");
    ObjectivePlan plan;
    const int rc = check_objective(m, batch, loss_type, false, plan);
    if (rc != DAD_OK) return rc;
    if (saved_bytes < plan.o.saved_bytes)
        return fail(DAD_E_WORKSPACE, "saved buffer has %zu bytes, the objective at batch %d needs %zu", saved_bytes, batch, plan.o.saved_bytes);
    return objective_forward_run(m, plan, x0, t_rows, noise, weights, loss_type, loss_out, batch, saved, stream);
}

int dad_train_objective_backward(dad_model* m, const float* x0, const float* noise, const float* weights, int32_t loss_type,
                                 const float* d_loss, float* const* grad_tensors, int32_t n_grad_tensors,
                                 float* const* time_grad_tensors, int32_t n_time_grad_tensors, int32_t batch, void* saved,
                                 size_t saved_bytes, void* scratch, size_t scratch_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!x0 || !noise || !d_loss || !grad_tensors || !time_grad_tensors || !saved || !scratch) return fail(DAD_E_INVALID, "null pointer");
    ObjectivePlan plan;
    const int rc = check_objective(m, batch, loss_type, true, plan);
    if (rc != DAD_OK) return rc;
    return objective_backward_run(m, plan, x0, noise, weights, loss_type, d_loss, grad_tensors, n_grad_tensors, time_grad_tensors,
                                  n_time_grad_tensors, batch, saved, saved_bytes, plan.o.saved_bytes, scratch, scratch_bytes,
                                  plan.o.scratch_bytes, stream, nullptr);
}

}  // extern "C"

namespace {

// Every refusal the dynamics-aware entry points add to check_objective's, in the order the header documents, and the plan
int check_dynamics(const dad_model* m, int batch, int loss_type, const dad_project_args* pa, int p_dim, int form, bool backward,
                   DynamicsObjectivePlan& plan) {
    if (loss_type != DAD_LOSS_L1 && loss_type != DAD_LOSS_L2)
        return fail(DAD_E_INVALID, "unknown loss_type %d (DAD_LOSS_L1 = 1, DAD_LOSS_L2 = 2)", loss_type);
    if (!m->training) return fail(DAD_E_INVALID, "training mode is off: dad_model_set_training(m, 1) before dad_model_finalize");
    if (m->precision != DAD_PREC_FP32) return fail(DAD_E_INVALID, "the training objective exists for the fp32 arithmetic only, not split-f16");
    if (batch <= 0) return fail(DAD_E_INVALID, "batch must be positive (got %d)", batch);
    if (!pa || !pa->P || !pa->obs_mean || !pa->obs_std || !pa->act_mean || !pa->act_std)
        return fail(DAD_E_INVALID, "dynamics objective: projection arguments missing");
    // (the shape before the state of the model: what dad_debug_dynamics_objective_plan refuses is refused here too)
    const int rc = dynamics_objective_plan(*m, batch, pa->state_dim, pa->observation_dim, pa->action_dim, form, backward, plan);
    if (plan.launches.empty()) return rc;
    if (p_dim != plan.D)
        return fail(DAD_E_INVALID, "dynamics objective: the projector is (%d, %d), horizon %d needs (%d, %d)", p_dim, p_dim, plan.horizon,
                    plan.D, plan.D);
    if (plan.vg.refused)
        return fail(DAD_E_INVALID, "dynamics objective: the row form at D=%d needs %zu bytes of LDS for one trajectory and its partial "
                    "sums (a CU has %zu); the GEMM form (form 1, or -1) takes any D", plan.D, plan.vg.fwd.lds_bytes, dad::kLdsBytes);
    if (!m->finalized) return fail(DAD_E_STATE, "dad_model_finalize has not been called");
    if (m->d_train_sched == nullptr) return fail(DAD_E_STATE, "dad_model_load_train_schedule has not been called");
    if (!m->have_sched) return fail(DAD_E_STATE, "schedule not loaded (dad_model_load_schedule)");
    return rc;
}

// the kernels' arguments: `q` as the fused objective's run filled it (forward: objective_params), the plan's regions
dad::DynamicsParams dynamics_params(const dad_model* m, const DynamicsObjectivePlan& plan, const dad::ObjectiveParams& q,
                                    const dad_project_args* pa, float diffusion_weight, float projection_weight,
                                    const float* timestep_weights, void* saved, void* scratch) {
    dad::DynamicsParams d{};
    const int T = m->cfg.n_timesteps, B = q.B;
    float* const sv = (float*)((char*)saved + plan.saved_base);
    const bool gemm = plan.vg.form == DAD_VG_GEMM;
    d.obj = q;
    dad::ProjParams& p = d.fwd.proj;
    p.P = pa->P; p.obs_mean = pa->obs_mean; p.obs_std = pa->obs_std; p.act_mean = pa->act_mean; p.act_std = pa->act_std;
    p.B = B; p.H = plan.horizon; p.n = pa->state_dim; p.od = pa->observation_dim; p.m = pa->action_dim; p.D = plan.D;
    p.alpha = 1.0f; p.one_minus_alpha = 0.0f;
    p.resid = sv + plan.r;
    p.violation = gemm ? nullptr : sv + plan.violation;
    d.fwd.part = gemm ? sv + plan.part : nullptr;
    d.fwd.col_blocks = plan.vg.col_blocks;
    dad::ViolationBwdParams& b = d.bwd;
    b.P = pa->P; b.obs_std = pa->obs_std; b.act_std = pa->act_std;
    b.r = sv + plan.r;
    b.g = gemm && scratch != nullptr ? (float*)((char*)scratch + plan.scratch_base) + plan.g : nullptr;
    b.B = B; b.H = plan.horizon; b.n = pa->state_dim; b.od = pa->observation_dim; b.m = pa->action_dim; b.D = plan.D;
    b.row_elems = q.row_elems;
    d.recip = m->d_recip_sched; d.recipm1 = m->d_recip_sched + T;
    d.tw = timestep_weights;
    d.diffusion_weight = diffusion_weight; d.projection_weight = projection_weight;
    d.bd = (float)((double)B * (double)plan.D);
    return d;
}

int launch_dynamics(const DynLaunch& l, const dad::DynamicsParams& d, hipStream_t st) {
    const dim3 grid(l.gx, l.gy), block((unsigned)l.threads);
    switch (l.kind) {
        case DAD_DO_K_FWD_ROW:
            if (l.rows_per_block == 1)
                hipLaunchKernelGGL((dad::dynamics_violation_fwd_row_kernel<1, dad::PROJ_KP>), grid, block, l.lds_bytes, st, d);
            else if (l.rows_per_block == 4)
                hipLaunchKernelGGL((dad::dynamics_violation_fwd_row_kernel<4, dad::PROJ_KP>), grid, block, l.lds_bytes, st, d);
            else return fail(DAD_E_STATE, "dynamics objective: %d trajectories per block planned", l.rows_per_block);
            break;
        case DAD_DO_K_FWD_GEMM: hipLaunchKernelGGL(dad::dynamics_violation_fwd_gemm_kernel, grid, block, l.lds_bytes, st, d); break;
        case DAD_DO_K_FWD_PARTS: hipLaunchKernelGGL(dad::dynamics_parts_kernel, grid, block, 0, st, d); break;
        case DAD_DO_K_BWD_ROW: hipLaunchKernelGGL(dad::dynamics_violation_bwd_row_kernel, grid, block, l.lds_bytes, st, d); break;
        case DAD_DO_K_BWD_GEMM: hipLaunchKernelGGL(dad::dynamics_violation_bwd_gemm_kernel, grid, block, l.lds_bytes, st, d); break;
        case DAD_DO_K_BWD_SCATTER: hipLaunchKernelGGL(dad::dynamics_scatter_dout_kernel, grid, block, 0, st, d); break;
        default: return fail(DAD_E_STATE, "dynamics objective: launch kind %d", l.kind);
    }
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

}  // namespace

extern "C" {

int dad_train_dynamics_objective_workspace_bytes(const dad_model* m, const dad_project_args* proj, int32_t form, int32_t batch,
                                                 size_t* saved_bytes, size_t* scratch_bytes) {
    if (!m || !proj) return fail(DAD_E_INVALID, "dynamics objective: null pointer");
    DynamicsObjectivePlan plan;
    const int rc = dynamics_objective_plan(*m, batch, proj->state_dim, proj->observation_dim, proj->action_dim, form, true, plan);
    if (plan.launches.empty()) return rc;      // (the shape was refused; a batch the pass refuses still has a size)
    if (saved_bytes) *saved_bytes = plan.saved_bytes;
    if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
    return DAD_OK;
}

int dad_train_dynamics_objective_forward(dad_model* m, const float* x0, const int32_t* t_rows, const float* noise,
                                         const float* weights, int32_t loss_type, const dad_project_args* proj, int32_t p_dim,
                                         int32_t form, float diffusion_weight, float projection_weight,
                                         const float* timestep_weights, float* parts, int32_t batch, void* saved,
                                         size_t saved_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!x0 || !t_rows || !noise || !parts || !saved) return fail(DAD_E_INVALID, "null pointer");
    DynamicsObjectivePlan plan;
    int rc = check_dynamics(m, batch, loss_type, proj, p_dim, form, false, plan);
    if (rc != DAD_OK) return rc;
    if (saved_bytes < plan.saved_bytes)
        return fail(DAD_E_WORKSPACE, "saved buffer has %zu bytes, the dynamics objective at batch %d needs %zu", saved_bytes, batch,
                    plan.saved_bytes);
    if ((rc = configure_kernels()) != DAD_OK || (rc = ensure_recip_schedule(m)) != DAD_OK) return rc;
    // the fused objective's own forward: parts[0] is its loss
    if ((rc = objective_forward_run(m, plan.obj, x0, t_rows, noise, weights, loss_type, parts, batch, saved, stream)) != DAD_OK) return rc;
    float* const sv = (float*)((char*)saved + plan.obj.o.saved_base);
    dad::ObjectiveParams q = objective_params(m, plan.obj.o, sv, batch, loss_type, x0, noise, weights);
    dad::DynamicsParams d = dynamics_params(m, plan, q, proj, diffusion_weight, projection_weight, timestep_weights, saved, nullptr);
    d.parts = parts;
    for (int i = 0; i < plan.fwd_launches; ++i)
        if ((rc = launch_dynamics(plan.launches[(size_t)i], d, (hipStream_t)stream)) != DAD_OK) return rc;
    return DAD_OK;
}

int dad_train_dynamics_objective_backward(dad_model* m, const float* x0, const float* noise, const float* weights, int32_t loss_type,
                                          const dad_project_args* proj, int32_t p_dim, int32_t form, float diffusion_weight,
                                          float projection_weight, const float* timestep_weights, const float* d_loss,
                                          float* const* grad_tensors, int32_t n_grad_tensors, float* const* time_grad_tensors,
                                          int32_t n_time_grad_tensors, int32_t batch, void* saved, size_t saved_bytes, void* scratch,
                                          size_t scratch_bytes, dad_stream_t stream) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    if (!x0 || !noise || !d_loss || !grad_tensors || !time_grad_tensors || !saved || !scratch) return fail(DAD_E_INVALID, "null pointer");
    DynamicsObjectivePlan plan;
    int rc = check_dynamics(m, batch, loss_type, proj, p_dim, form, true, plan);
    if (rc != DAD_OK) return rc;
    if ((rc = configure_kernels()) != DAD_OK || (rc = ensure_recip_schedule(m)) != DAD_OK) return rc;
    // d total / d out: the violation backward, whose scatter epilogue adds the diffusion term's gradient, in place of
    // objective_dout_kernel
    const std::function<int(const dad::ObjectiveParams&)> head = [&](const dad::ObjectiveParams& q) -> int {
        const dad::DynamicsParams d = dynamics_params(m, plan, q, proj, diffusion_weight, projection_weight, timestep_weights, saved, scratch);
        for (size_t i = (size_t)plan.fwd_launches; i < plan.launches.size(); ++i) {
            const int lrc = launch_dynamics(plan.launches[i], d, (hipStream_t)stream);
            if (lrc != DAD_OK) return lrc;
        }
        return DAD_OK;
    };
    return objective_backward_run(m, plan.obj, x0, noise, weights, loss_type, d_loss, grad_tensors, n_grad_tensors, time_grad_tensors,
                                  n_time_grad_tensors, batch, saved, saved_bytes, plan.saved_bytes, scratch, scratch_bytes,
                                  plan.scratch_bytes, stream, &head);
}


int dad_fill_normal(float* x, int32_t batch, int32_t row_elems, uint64_t seed, uint64_t row_offset,
                    uint64_t draw, dad_stream_t stream) {
    if (!x || batch <= 0 || row_elems <= 0) return fail(DAD_E_INVALID, "bad argument");
    const long n = (long)batch * row_elems;
    hipLaunchKernelGGL(dad::fill_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, x, n, row_offset * (uint64_t)row_elems, draw, seed);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

#ifdef DAD_STAMPS
int dad_debug_stamps(void* buf) { g_stamps = (unsigned long long*)buf; return DAD_OK; }
#endif
// 1 when the generated registry holds, for every family, an entry wherever the family's predicate is true over its
// domain, the family's count of them, and nothing else
int dad_debug_kernel_table_consistent(void) {
    size_t hits = 0;
    for (int fam = 0; fam < kNumFamilies; ++fam) {
        const FamilyDomain& d = kFamilies[fam];
        int n = 0;
        for (int i = 0; i < family_domain_size(fam); ++i) {
            int k[kMaxKeyInts] = {};
            family_key_at(fam, i, k);
            const bool have = find_kernel(fam, k, d.axes) != nullptr;
            if (have != family_kernel_exists(fam, k)) {
                fail(DAD_E_INVALID, "kernel table mismatch: %s key (%d, %d, %d, %d, %d, %d)[:%d] (registry %d)", d.name, k[0], k[1], k[2], k[3],
                     k[4], k[5], d.axes, (int)have);
                return 0;
            }
            if (fam == FAM_HALO8 && have != (find_halo8w(k[0], k[1] != 0) != nullptr)) {     // both forms of every key
                fail(DAD_E_INVALID, "kernel table mismatch: conv_halo8w_f32 key (%d, %d) (registry %d)", k[0], k[1], (int)have);
                return 0;
            }
            n += have;
        }
        if (n != d.count) {
            fail(DAD_E_INVALID, "kernel table mismatch: %d %s kernels, expected %d", n, d.name, d.count);
            return 0;
        }
        hits += (size_t)n;
    }
    if (hits != kernel_table().size()) {      // an entry outside every domain, or one key twice
        fail(DAD_E_INVALID, "kernel table mismatch: %zu entries, %zu inside the families' domains", kernel_table().size(), hits);
        return 0;
    }
    return 1;
}

int dad_debug_kernel_list(int32_t family, int32_t* out, int32_t capacity, int32_t* needed_out) {
    if (family < 0 || family >= kNumFamilies || capacity < 0 || (capacity > 0 && !out)) return fail(DAD_E_INVALID, "bad argument");
    const int axes = kFamilies[family].axes;
    std::vector<int32_t> r(DAD_KL_HEADER, 0);
    r[DAD_KL_KEY_INTS] = axes;
    for (const KernelEntry& e : kernel_table()) {
        if ((int)(e.key >> (8 * kMaxKeyInts)) != family) continue;
        for (int a = 0; a < axes; ++a) r.push_back((int32_t)(e.key >> (8 * (kMaxKeyInts - 1 - a)) & 0xff));
        ++r[DAD_KL_KERNELS];
    }
    return copy_report(r, out, capacity, needed_out);
}

const char* dad_debug_report_layout(int32_t report, int32_t section) { return report_layout(report, section); }

#ifdef DAD_WG_STAMPS
extern "C" int dad_debug_wgrad_stamps(unsigned long long* host32) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(host32, HIP_SYMBOL(dad::g_wg_stamps), 32 * sizeof(unsigned long long)));
    return DAD_OK;
}
#endif

int dad_debug_set_tile(dad_model* m, int32_t cfg) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    // cfg >= 100: same, with grid-level split-K disabled (cfg - 100 is the tile, 99 = heuristic)
    m->split_enabled = cfg < 99;
    m->force_tile = cfg >= 99 ? cfg - 100 : cfg;
    return DAD_OK;
}

int dad_debug_set_option(dad_model* m, const char* name, int32_t value) {
    if (!m || !name) return fail(DAD_E_INVALID, "null argument");
    const std::string key(name);
    if (key == "fuse_residual") m->fuse_residual = value != 0;
    else if (key == "xswz") m->xswz_enabled = value != 0;
    else if (key == "xcd_order") m->xcd_order = value != 0;
    else if (key == "split_target") m->split_target = std::max(1, (int)value);
    else if (key == "cc") m->cc_enabled = value != 0;
    else if (key == "cc_max_rows") m->cc_max_rows = std::max(0, (int)value);
    else if (key == "ccw_max_rows") m->ccw_max_rows = std::max(0, (int)value);
    else if (key == "ccw_min_blocks") m->ccw_min_blocks = std::max(1, (int)value);
    else if (key == "ccw_prefer16") m->ccw_prefer16 = value != 0;
    else if (key == "wgrad_blocks") m->wgrad_blocks = std::max(1, (int)value);
    else if (key == "halo8") m->halo8_enabled = value != 0;
    else if (key == "halo8_wreg") m->halo8_wreg = value < 0 ? -1 : value != 0;
    else if (key == "step_seam") m->step_seam = value != 0;
    else return fail(DAD_E_INVALID, "unknown option '%s'", name);
    // every option changes which launches a captured loop holds, and not all of them are part of the
    // graph key: drop the cache (a replay may still be in flight: wait for the device first)
    if (!m->graphs.empty()) {
        HIP_TRY(hipDeviceSynchronize());
        for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
        m->graphs.clear();
    }
    return DAD_OK;
}

int dad_debug_read_table(dad_model* m, int32_t which, int32_t t, float* host_out, int32_t capacity,
                         int32_t* width_out) {
    if (!m || !host_out) return fail(DAD_E_INVALID, "null argument");
    if (!m->finalized) return fail(DAD_E_STATE, "dad_model_finalize has not been called");
    if (t < 0 || t >= m->cfg.n_timesteps)
        return fail(DAD_E_RANGE, "index %d is out of bounds for the schedule of size %d", t, m->cfg.n_timesteps);
    { const int rc = ensure_tables(m, nullptr); if (rc != DAD_OK) return rc; }      // (null stream: the copy below follows it)
    const float* base = nullptr;
    int width = 0;
    switch (which) {
        case DAD_TABLE_SINUSOID: base = m->d_emb; width = m->cfg.dim; break;
        case DAD_TABLE_TIME_MLP: base = m->d_temb; width = m->cfg.time_dim; break;
        case DAD_TABLE_BLOCKS: base = m->d_temb_table; width = m->plan.temb_width; break;
        default: return fail(DAD_E_INVALID, "unknown table %d", which);
    }
    if (width_out) *width_out = width;
    if (capacity < width)
        return fail(DAD_E_INVALID, "table %d has rows of %d floats, the buffer holds %d", which, width, capacity);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, base + (size_t)t * width, (size_t)width * sizeof(float), hipMemcpyDeviceToHost));
    return DAD_OK;
}

int dad_debug_mish(const float* in, float* out, int64_t n, dad_stream_t stream) {
    if (!in || !out || n <= 0) return fail(DAD_E_INVALID, "bad argument");
    hipLaunchKernelGGL(dad::mish_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, in, out, (long)n);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

int dad_debug_small_batch_plan(dad_model* m, int32_t batch, int32_t* launches_out, int32_t* wide_out) {
    if (!m || batch <= 0) return fail(DAD_E_INVALID, "bad argument");
    const CcPlan cc = cc_plan(*m, batch);
    int launches = 0, wide = 0;
    if (cc.ok)
        for (const CcOp& o : cc.ops) {
            launches += o.launched;
            wide += o.launched && o.wide;
        }
    static const bool trace = getenv("DAD_TRACE_TILES") != nullptr;
    if (trace && !cc.ok) fprintf(stderr, "[dad] batch %d: no small-batch plan (%s)\n", batch, cc.why.c_str());
    if (launches_out) *launches_out = launches;
    if (wide_out) *wide_out = wide;
    return DAD_OK;
}

int dad_debug_backward_plan(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out) {
    return training_report(m, batch, backward_plan_report, out, capacity, needed_out);
}

int dad_debug_backward_steps(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out) {
    return training_report(m, batch, backward_steps_report, out, capacity, needed_out);
}

int dad_debug_objective_plan(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out) {
    return training_report(m, batch, objective_plan_report, out, capacity, needed_out);
}

int dad_debug_dynamics_objective_plan(dad_model* m, int32_t batch, int32_t state_dim, int32_t observation_dim, int32_t action_dim,
                                      int32_t form, int32_t* out, int32_t capacity, int32_t* needed_out) {
    if (!m || capacity < 0 || (capacity > 0 && !out)) return fail(DAD_E_INVALID, "bad argument");
    if (!m->training) return fail(DAD_E_STATE, "dad_model_set_training(m, 1) has not been called");
    if (m->bwd_rc != DAD_OK) return fail(m->bwd_rc, "%s", m->bwd_err.c_str());
    std::vector<int32_t> r;
    const int rc = dynamics_objective_plan_report(*m, batch, state_dim, observation_dim, action_dim, form, r);
    return rc != DAD_OK ? rc : copy_report(r, out, capacity, needed_out);
}

int dad_debug_forward_plan(dad_model* m, int32_t batch, int32_t mode, int32_t* out, int32_t capacity, int32_t* needed_out) {
    if (!m || batch <= 0 || mode < 0 || mode > 3 || capacity < 0 || (capacity > 0 && !out)) return fail(DAD_E_INVALID, "bad argument");
    if (mode >= 2 && !m->training) return fail(DAD_E_STATE, "dad_model_set_training(m, 1) has not been called");
    if (mode == 3 && m->bwd_rc != DAD_OK) return fail(m->bwd_rc, "%s", m->bwd_err.c_str());
    std::vector<int32_t> r;
    const int rc = forward_plan_report(*m, batch, mode, r);     // (a batch the call refuses is refused here too)
    return rc != DAD_OK ? rc : copy_report(r, out, capacity, needed_out);
}

int dad_debug_halo8_plan(dad_model* m, int32_t batch, int32_t mode, int32_t* out, int32_t capacity, int32_t* needed_out) {
    if (!m || batch <= 0 || mode < 0 || mode > 1 || capacity < 0 || (capacity > 0 && !out)) return fail(DAD_E_INVALID, "bad argument");
    FwdPlan f;
    const int rc = plan_forward(*m, false, batch, mode == 0, f);     // (as dad_debug_forward_plan plans modes 0 / 1)
    if (rc != DAD_OK) return rc;
    std::vector<int32_t> r;
    halo8_plan_encode(*m, f, mode == 1, r);
    return copy_report(r, out, capacity, needed_out);
}

int dad_debug_project_plan(int32_t state_dim, int32_t observation_dim, int32_t action_dim, int32_t batch, int32_t horizon,
                           size_t scratch_bytes, int32_t violation, int32_t* out) {
    if (!out || state_dim <= 0 || observation_dim < state_dim || action_dim <= 0 || batch <= 0 || horizon <= 0)
        return fail(DAD_E_INVALID, "bad argument");
    return project_plan_report(state_dim, observation_dim, action_dim, batch, horizon, scratch_bytes, violation != 0, out);
}

int dad_debug_violation_grad_plan(int32_t state_dim, int32_t observation_dim, int32_t action_dim, int32_t batch, int32_t horizon,
                                  int32_t form, int32_t* out) {
    if (!out) return fail(DAD_E_INVALID, "violation gradient: null pointer");
    return violation_grad_plan_report(state_dim, observation_dim, action_dim, batch, horizon, form, out);
}

int dad_debug_seam_plan(dad_model* m, int32_t batch, int32_t projection, int32_t* out) {
    if (!m || !out || batch <= 0) return fail(DAD_E_INVALID, "bad argument");
    return seam_plan_report(*m, batch, projection != 0, out);
}

int dad_debug_guide_plan(int32_t in_dim, const int32_t* widths, int32_t n_layers, int32_t activation, int32_t batch,
                         int32_t horizon, int32_t transition_dim, int32_t* out) {
    if (!out || (!widths && n_layers > 0)) return fail(DAD_E_INVALID, "guide: null pointer");
    return guide_plan_report(in_dim, widths, n_layers, activation, batch, horizon, transition_dim, out);
}

const char* dad_debug_seam_reason(int32_t reason) { return seam_reason(reason); }

int dad_profile_enable(dad_model* m, int32_t on) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    m->profile = on != 0;
    m->ev_used = 0;
    m->prof_flops = 0;
    m->prof_launches = 0;
    return DAD_OK;
}

int dad_profile_read(dad_model* m, double* conv_ms, int64_t* conv_launches, double* conv_flops) {
    if (!m) return fail(DAD_E_INVALID, "null model");
    double ms = 0;
    for (size_t i = 0; i < m->ev_used; ++i) {
        HIP_TRY(hipEventSynchronize(m->ev_pool[i].second));
        float d = 0;
        HIP_TRY(hipEventElapsedTime(&d, m->ev_pool[i].first, m->ev_pool[i].second));
        ms += d;
    }
    if (conv_ms) *conv_ms = ms;
    if (conv_launches) *conv_launches = m->prof_launches;
    if (conv_flops) *conv_flops = m->prof_flops;
    m->ev_used = 0;
    m->prof_flops = 0;
    m->prof_launches = 0;
    return DAD_OK;
}

}  // extern "C"  (the optimiser step follows)

// ------------------------------------------------------------------ the optimiser step (csrc/optim_step.hpp)
// The device table of a step: n descriptors, then first[n + 1] of the plan.  `image` is its host copy as last
// uploaded; a step whose table equals it launches straight away.  An upload copies the table into a pinned staging
// buffer nobody is reading (each buffer carries an event recorded behind its last copy; a buffer whose event has not
// completed is left alone and another one is made) and enqueues the copy on the caller's stream, where it runs
// behind the previous step's kernels: no synchronisation.  A table that outgrows its device buffer gets a new one;
// the old one is freed with the object (a step still in flight may read it).
struct dad_optim {
    struct Stage { void* host; size_t cap; hipEvent_t done; };
    std::vector<Stage> stages;
    std::vector<void*> owned;             // device allocations
    void* d_table = nullptr;
    size_t table_cap = 0;
    double* d_partials = nullptr;         // kOptimMaxGrid partial square sums
    std::vector<char> image;
    std::vector<int64_t> numel;           // sizes `plan` was made for
    OptimPlan plan;
};

namespace {

int optim_upload(dad_optim* o, const std::vector<char>& image, hipStream_t st) {
    const size_t bytes = image.size();
    if (o->table_cap < bytes) {
        void* a = nullptr;
        HIP_TRY(hipMalloc(&a, bytes * 2));
        o->owned.push_back(a);
        o->d_table = a;
        o->table_cap = bytes * 2;
    }
    dad_optim::Stage* use = nullptr;
    for (auto& sg : o->stages) {
        if (sg.cap < bytes) continue;
        const hipError_t q = hipEventQuery(sg.done);
        if (q == hipSuccess) { use = &sg; break; }
        if (q != hipErrorNotReady) return fail(DAD_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
        (void)hipGetLastError();          // (not ready is no error of this call)
    }
    if (!use) {
        dad_optim::Stage sg{nullptr, bytes * 2, nullptr};
        HIP_TRY(hipHostMalloc(&sg.host, sg.cap, hipHostMallocDefault));
        const hipError_t e = hipEventCreateWithFlags(&sg.done, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipHostFree(sg.host);
            return fail(DAD_E_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        o->stages.push_back(sg);
        use = &o->stages.back();
    }
    std::memcpy(use->host, image.data(), bytes);
    HIP_TRY(hipMemcpyAsync(o->d_table, use->host, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(use->done, st));
    return DAD_OK;
}

}  // namespace

extern "C" {

int dad_optim_create(dad_optim** out) {
    if (!out) return fail(DAD_E_INVALID, "null out");
    *out = new dad_optim();
    return DAD_OK;
}

void dad_optim_destroy(dad_optim* o) {
    if (!o) return;
    for (auto& sg : o->stages) { (void)hipEventDestroy(sg.done); (void)hipHostFree(sg.host); }
    for (void* p : o->owned) (void)hipFree(p);
    delete o;
}

int dad_optim_step(dad_optim* o, const dad_optim_tensor* tensors, int32_t n, const dad_optim_args* a, dad_stream_t s) {
    if (!o || !tensors || !a) return fail(DAD_E_INVALID, "optimiser step: null %s", !o ? "dad_optim" : !tensors ? "tensor list" : "arguments");
    if (n <= 0) return fail(DAD_E_INVALID, "optimiser step: n = %d tensors", n);
    if (!a->groups) return fail(DAD_E_INVALID, "optimiser step: null groups");
    if (a->n_groups <= 0 || a->n_groups > kOptimMaxGroups)
        return fail(DAD_E_INVALID, "optimiser step: %d groups (1 .. %d)", a->n_groups, kOptimMaxGroups);
    bool any_grad = false, same_numel = o->numel.size() == (size_t)n;
    for (int i = 0; i < n; ++i) {
        const dad_optim_tensor& t = tensors[i];
        if (!t.param) return fail(DAD_E_INVALID, "optimiser step: tensor %d has a null param", i);
        if (t.numel <= 0) return fail(DAD_E_INVALID, "optimiser step: tensor %d has numel %lld", i, (long long)t.numel);
        if (t.group < 0 || t.group >= a->n_groups)
            return fail(DAD_E_INVALID, "optimiser step: tensor %d is in group %d of %d", i, t.group, a->n_groups);
        if (t.grad && (!t.exp_avg || !t.exp_avg_sq))
            return fail(DAD_E_INVALID, "optimiser step: tensor %d has a grad but no %s", i, !t.exp_avg ? "exp_avg" : "exp_avg_sq");
        if (!t.grad && !t.ema) return fail(DAD_E_INVALID, "optimiser step: tensor %d has neither grad nor ema: nothing to do", i);
        any_grad = any_grad || t.grad;
        same_numel = same_numel && o->numel[(size_t)i] == t.numel;
    }
    if (!same_numel) {
        std::vector<int64_t> numel((size_t)n);
        for (int i = 0; i < n; ++i) numel[(size_t)i] = tensors[i].numel;
        OptimPlan p;
        const int rc = optim_plan(numel.data(), n, p);
        if (rc != DAD_OK) return rc;
        o->plan = std::move(p);
        o->numel = std::move(numel);
    }
    hipStream_t st = (hipStream_t)s;
    const size_t desc_bytes = (size_t)n * sizeof(dad::OptimDesc), first_bytes = o->plan.first.size() * sizeof(int32_t);
    std::vector<char> image(desc_bytes + first_bytes, 0);
    for (int i = 0; i < n; ++i) {
        const dad_optim_tensor& t = tensors[i];
        dad::OptimDesc d{};                // (built in place: padding bytes stay zero for the comparison)
        d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq; d.ema = t.ema;
        d.numel = t.numel; d.group = t.group;
        const uintptr_t bits = (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq | (uintptr_t)t.ema;
        d.vec = (bits & 15) == 0;
        std::memcpy(image.data() + (size_t)i * sizeof(dad::OptimDesc), &d, sizeof(d));
    }
    std::memcpy(image.data() + desc_bytes, o->plan.first.data(), first_bytes);
    if (image != o->image) {
        const int rc = optim_upload(o, image, st);
        if (rc != DAD_OK) { o->image.clear(); return rc; }
        o->image.swap(image);
    }
    if (!o->d_partials) {
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, kOptimMaxGrid * sizeof(double)));
        o->owned.push_back(p);
        o->d_partials = (double*)p;
    }
    const auto* descs = (const dad::OptimDesc*)o->d_table;
    const int* first = (const int*)((const char*)o->d_table + desc_bytes);
    const OptimGeom g = o->plan.g;
    const bool norm = any_grad && (a->max_grad_norm > 0.f || a->grad_norm_out);
    if (!any_grad && a->grad_norm_out)      // nothing to sum: the norm of no gradients is 0, as clip_grad_norm_ gives
        HIP_TRY(hipMemsetAsync(a->grad_norm_out, 0, sizeof(float), st));
    if (norm) {
        hipLaunchKernelGGL(dad::optim_sqsum_kernel, dim3((unsigned)g.grid), dim3(dad::OPT_THREADS), 0, st, descs, first, (int)n, g,
                           o->d_partials);
        HIP_TRY(hipGetLastError());
    }
    dad::OptimGroups groups{};
    std::copy(a->groups, a->groups + a->n_groups, groups.g);
    hipLaunchKernelGGL(dad::optim_update_kernel, dim3((unsigned)g.grid), dim3(dad::OPT_THREADS), 0, st, descs, first, (int)n, g,
                       groups, (const double*)o->d_partials, norm ? g.grid : 0, a->max_grad_norm, a->ema_decay, a->grad_norm_out);
    HIP_TRY(hipGetLastError());
    return DAD_OK;
}

int dad_debug_optim_plan(const int64_t* numel, int32_t n, int32_t* out, int32_t capacity, int32_t* needed_out) {
    if (!numel || n <= 0 || capacity < 0 || (capacity > 0 && !out)) return fail(DAD_E_INVALID, "bad argument");
    std::vector<int32_t> r;
    const int rc = optim_plan_report(numel, n, r);
    return rc != DAD_OK ? rc : copy_report(r, out, capacity, needed_out);
}

}  // extern "C"
