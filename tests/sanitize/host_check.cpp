// host_check.cpp — the host logic of libdad_hip.so (csrc/host_plan.hpp: architecture checks, launch
// plan, workspace layout, weight packing incl. split-f16 images, tile choice, grid split-K, LDS slot
// shifts, launch geometry) compiled WITHOUT HIP under -fsanitize=address,undefined and driven over
// the five architectures of the parity tests plus a deterministic sweep of the fuzz generator's
// space (tests/fuzz_parity.py).  Besides what the sanitizers catch, every launch is checked against
// the invariants the kernels assume.  Built and run by tests/test_host_logic.py (CPU suite); GPU
// sanitizers are not used anywhere.
#include <cinttypes>
#include <cstdio>
#include <random>

#include "../../dynamics_aware_diffusion_amd/csrc/host_plan.hpp"

using namespace dadhost;

// The report layouts of include/dad.h against literal offsets (independent of dad_debug_report_layout, which
// tests/test_host_logic.py holds against tests/golden/report_layouts.json): per report the first and the last field, the
// lengths, and the four fields that span more than one int.
static_assert(DAD_FP_MODE == 0 && DAD_FP_FINAL_KERNEL == 7 && DAD_FP_HEADER == 8 && DAD_FP_REC_CONV == 0 && DAD_FP_REC_FAMILY == 12 &&
              DAD_FP_REC_INTS == 13 && DAD_FP_CC_CONV == 0 && DAD_FP_CC_RES_KIND == 12 && DAD_FP_CC_INTS == 13, "DAD_FP_*");
static_assert(DAD_H8_HEADER == 2 && DAD_H8_CONV == 0 && DAD_H8_PART_TILE == 13 && DAD_H8_INTS == 14, "DAD_H8_*");
static_assert(DAD_SEAM_TAKEN == 0 && DAD_SEAM_TILE0 == 11 && DAD_SEAM_INTS == 12 && DAD_SEAM_BUF_RDST == 2, "DAD_SEAM_*");
static_assert(DAD_PP_FORM == 0 && DAD_PP_REFUSED == 5 && DAD_PP_INTS == 6 && DAD_PP_GEMM == 2, "DAD_PP_*");
static_assert(DAD_BP_WGRADS == 0 && DAD_BP_TILE == 7 && DAD_BP_TAPS_TILE == 11 && DAD_BP_FWD == 31 && DAD_BP_DGRAD == 51 &&
              DAD_BP_RECORD_INTS == 71 && DAD_BP_HEADER == 72 && DAD_BP_REC_TAPS == 0 && DAD_BP_REC_LAST_CHUNKS == 8 && DAD_BP_REC_INTS == 9,
              "DAD_BP_*");
static_assert(DAD_BS_STEPS == 0 && DAD_BS_DX == 9 && DAD_BS_HEADER == 12 && DAD_BS_KIND == 0 && DAD_BS_BIAS_ROWS == 1 && DAD_BS_WG_TAPS == 1 &&
              DAD_BS_WG_LAST_CHUNKS == 24 && DAD_BS_DG_WRITE == 3 && DAD_BS_GN_C == 8 && DAD_BS_RS_TO_X == 3 && DAD_BS_CL_WRITE == 5 &&
              DAD_BS_REC_INTS == 25 && DAD_BS_K_COLS == 5, "DAD_BS_*");
static_assert(DAD_OP_LOSS_BLOCKS == 0 && DAD_OP_LAUNCHES == 7 && DAD_OP_HEADER == 8 && DAD_OP_REC_MODE == 0 && DAD_OP_REC_KSLICE == 10 &&
              DAD_OP_REC_INTS == 11 && DAD_OP_TG_DTEMB == 8, "DAD_OP_*");
static_assert(DAD_OS_CHUNK == 0 && DAD_OS_RECORD_INTS == 4 && DAD_OS_HEADER == 5 && DAD_OS_REC_TENSOR == 0 && DAD_OS_REC_BLOCK == 4 &&
              DAD_OS_REC_INTS == 5, "DAD_OS_*");
static_assert(DAD_FAMILY_GEMM == 0 && DAD_FAMILY_WGRAD == 5 && DAD_FAMILIES == 6, "DAD_FAMILY_*");

static int g_failures = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            ++g_failures;                                                      \
            fprintf(stderr, "CHECK failed %s:%d: %s — ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
        }                                                                      \
    } while (0)

struct Arch {
    const char* name;
    int td, dim, time_dim, horizon;
    std::vector<int> mults;
    bool pack;      // also load synthetic weights and build the packed images
    int ks = 5;     // TemporalUnet(kernel_size): 3, 5 or 7
    std::vector<int> real = {};   // dad_model_set_group_channels: level widths before zero-padding the groups
    int hreal = 0;                // dad_model_set_horizon: horizon before zero-padding (0: as given)
};

static float synth(uint64_t& state) {       // cheap deterministic values in (-1, 1)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((int64_t)(state >> 33) - (1ll << 30)) / (float)(1ll << 30);
}

// the conflict condition find_xswz promises, re-checked independently for the shifts it returns
static bool xswz_conflict_free(uint64_t packed, int L, int stride, int pad, int kp4, int BN) {
    static const int groups[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    const int seg = L * stride + 2 * pad;
    for (int tn = 0; tn < BN / 32; ++tn)
        for (const auto& g : groups) {
            unsigned seen = 0;
            for (int lane : g) {
                const int n = tn * 32 + lane, sm = n / L, l = n % L;
                const int d = (int)((packed >> (4 * sm)) & 15);
                const unsigned bit = 1u << (((sm * seg + l * stride) * kp4 + d) & 15);
                if (seen & bit) return false;
                seen |= bit;
            }
        }
    return true;
}

// The packed layouts stated a second time, independently of weight_image.hpp: explicit loops over the source
// tensors.  Every image of the weight table must equal them bit for bit.
// Conv1d weight (co, ci, k)  ->  [ci_pad/KC][wtaps][M = co][KC]; tap index `tap_at + t`.
static void ref_pack_conv_into(std::vector<float>& out, const HostTensor& w, int wtaps, int tap_at, int kc) {
    const int co = (int)w.shape[0], ci = (int)w.shape[1], k = (int)w.shape[2];
    for (int o = 0; o < co; ++o)
        for (int i = 0; i < ci; ++i)
            for (int t = 0; t < k; ++t) {
                const size_t row = ((size_t)(i / kc) * wtaps + tap_at + t) * co + o;
                out[row * kc + (i % kc)] = w.data[((size_t)o * ci + i) * k + t];
            }
}
// ConvTranspose1d weight (ci, co, 4), stride 2, pad 1, as a 2-tap conv with M = 2*co columns:
//   y[co, 2j]   = sum_ci W[ci,co,3] x[ci,j-1] + W[ci,co,1] x[ci,j]       columns [0, co)
//   y[co, 2j+1] = sum_ci W[ci,co,2] x[ci,j]   + W[ci,co,0] x[ci,j+1]     columns [co, 2co)
static std::vector<float> ref_pack_convT(const HostTensor& w, int cin_pad, int kc) {
    const int ci = (int)w.shape[0], co = (int)w.shape[1];
    const int M = 2 * co;
    std::vector<float> out((size_t)cin_pad * 2 * M, 0.0f);
    auto at = [&](int i, int o, int kk) { return w.data[((size_t)i * co + o) * 4 + kk]; };
    for (int i = 0; i < ci; ++i)
        for (int o = 0; o < co; ++o) {
            auto slot = [&](int tap, int mm) -> float& {
                return out[(((size_t)(i / kc) * 2 + tap) * M + mm) * kc + (i % kc)];
            };
            slot(0, o) = at(i, o, 3);
            slot(1, o) = at(i, o, 1);
            slot(0, co + o) = at(i, o, 2);
            slot(1, co + o) = at(i, o, 0);
        }
    return out;
}
// forward image of a conv (fp32)
static std::vector<float> ref_fwd_image(const HostModel& m, const ConvOp& op) {
    const int pack_g = op.bdir ? 16 : op.kc;
    const HostTensor& w = m.raw.at(op.name + ".weight");
    if (op.kind == CONV_UP) return ref_pack_convT(w, op.cin_pad, pack_g);
    std::vector<float> out((size_t)op.cin_pad * op.wtaps() * op.M, 0.0f);
    ref_pack_conv_into(out, w, op.wtaps(), 0, pack_g);
    if (op.ride) ref_pack_conv_into(out, m.raw.at(op.rname + ".weight"), op.wtaps(), op.taps, pack_g);
    return out;
}
// image of data-gradient launch s of forward conv f: the equivalent conv's weight tensor, then packed
static std::vector<float> ref_bwd_image(const HostModel& m, const ConvOp& f, const HostModel::BwdConv& b, int s) {
    const HostTensor& w = m.raw.at(f.name + ".weight");
    const ConvOp& op = b.op[s];
    const int cin = f.cin0 + f.cin1;
    HostTensor t;
    std::vector<float> out;
    if (f.kind == CONV_K5 || f.kind == CONV_1X1) {
        const int K = f.taps;
        t.shape = {op.cout, f.cout, K};
        t.data.assign((size_t)op.cout * f.cout * K, 0.0f);
        for (int mm = 0; mm < b.c_n[s]; ++mm)
            for (int co = 0; co < f.cout; ++co)
                for (int k = 0; k < K; ++k)
                    t.data[((size_t)mm * f.cout + co) * K + k] = w.data[((size_t)co * cin + b.c_lo[s] + mm) * K + (K - 1 - k)];
        out.assign((size_t)op.cin_pad * K * op.M, 0.0f);
        ref_pack_conv_into(out, t, K, 0, 16);
    } else if (f.kind == CONV_DOWN) {            // -> transposed conv (in = co, out = ci, 4 taps; tap 3 zero)
        t.shape = {f.cout, cin, 4};
        t.data.assign((size_t)f.cout * cin * 4, 0.0f);
        for (int co = 0; co < f.cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int k = 0; k < 3; ++k)
                    t.data[((size_t)co * cin + ci) * 4 + k] = w.data[((size_t)co * cin + ci) * 3 + k];
        out = ref_pack_convT(t, op.cin_pad, 16);
    } else {                                     // CONV_UP -> 5-tap stride-2 conv (out = ci, in = co; tap 0 zero)
        t.shape = {cin, f.cout, 5};
        t.data.assign((size_t)cin * f.cout * 5, 0.0f);
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < f.cout; ++co)
                for (int kk = 0; kk < 4; ++kk)
                    t.data[((size_t)ci * f.cout + co) * 5 + kk + 1] = w.data[((size_t)ci * f.cout + co) * 4 + kk];
        out.assign((size_t)op.cin_pad * 5 * op.M, 0.0f);
        ref_pack_conv_into(out, t, 5, 0, 16);
    }
    return out;
}
static std::vector<float> ref_bfinal_image(const HostModel& m) {
    const HostTensor& w = m.raw.at("final_conv.1.weight");            // (td, dim, 1)
    const int td = m.cfg.transition_dim, dim = m.cfg.dim;
    HostTensor t;
    t.shape = {dim, td, 1};
    t.data.assign((size_t)dim * td, 0.0f);
    for (int j = 0; j < td; ++j)
        for (int c = 0; c < dim; ++c) t.data[(size_t)c * td + j] = w.data[(size_t)j * dim + c];
    std::vector<float> out((size_t)m.bfinal.cin_pad * m.bfinal.M, 0.0f);
    ref_pack_conv_into(out, t, 1, 0, 16);
    return out;
}

// dad_debug_forward_plan: the report must say what the description it was read from says — every field of every launch, in
// order, and the kernel its flag word names must be the one launch_conv looks up (and must exist).  `f`: modes 0 .. 2,
// `ts`: mode 3.  Counts the reports it compared.
static long g_reports = 0;
static void check_forward_report(const HostModel& m, int mode, int B, const FwdPlan* f, const TrainScratch* ts, int rc_plan) {
    std::vector<int32_t> r;
    const int rc = forward_plan_report(m, B, mode, r);
    CHECK(rc == rc_plan, "mode %d B=%d: the plan report returns %d, the description %d", mode, B, rc, rc_plan);
    CHECK(r.size() >= DAD_FP_HEADER && r[DAD_FP_MODE] == mode && r[DAD_FP_BATCH] == B, "mode %d B=%d: report header", mode, B);
    if (r.size() < DAD_FP_HEADER) return;
    const int n = r[DAD_FP_RECORDS], ints = r[DAD_FP_RECORD_INTS];
    CHECK(r.size() == (size_t)DAD_FP_HEADER + (size_t)n * ints, "mode %d B=%d: %zu ints for %d records of %d", mode, B, r.size(), n, ints);
    if (r.size() != (size_t)DAD_FP_HEADER + (size_t)n * ints) return;
    ++g_reports;
    auto conv = [&](const int32_t* q, int index, int sub, const ConvOp& op, const LaunchGeom& g, bool ok) {
        const int fl = q[DAD_FP_REC_FLAGS];
        CHECK(q[DAD_FP_REC_CONV] == index && q[DAD_FP_REC_SUB] == sub && q[DAD_FP_REC_CFG] == g.cfg && q[DAD_FP_REC_TAPS] == op.taps &&
              q[DAD_FP_REC_STRIDE] == op.stride && q[DAD_FP_REC_KC] == g.kc && q[DAD_FP_REC_KSLICES] == g.split.kslices &&
              q[DAD_FP_REC_GN_NPT] == g.gn_npt && q[DAD_FP_REC_NTILES_N] == g.ntiles_n && q[DAD_FP_REC_MTILES] == g.mtiles,
              "%s mode %d B=%d: report record differs from the launch", op.name.c_str(), mode, B);
        CHECK(((fl & 1) != 0) == op.x3 && ((fl & 2) != 0) == op.bdir && ((fl & 4) != 0) == g.ragged && ((fl & 8) != 0) == g.fused &&
              ((fl & 16) != 0) == g.padded && ((fl & 32) != 0) == g.windowed && fl < (1 << kRegFlags),
              "%s mode %d B=%d: flag word %d", op.name.c_str(), mode, B, fl);
        if (!ok) return;
        CHECK(kernel_registered_f(g.cfg, op.taps, op.stride, fl) && family_kernel_exists(FAM_GEMM, {g.cfg, op.taps, op.stride, fl}) &&
              kernel_registered(g.cfg, op.taps, op.stride, op.x3, op.bdir, g.ragged, g.fused, g.padded, g.windowed),
              "%s mode %d B=%d: the report names a kernel that does not exist", op.name.c_str(), mode, B);
        // samples the launch's N tiles have room for against the batch
        const TileCfg& t = kTiles[g.cfg];
        const long room = op.Lout > t.BN ? B : (long)g.ntiles_n * (t.BN / op.Lout);
        CHECK((q[DAD_FP_REC_PART_TILE] != 0) == (room != B), "%s mode %d B=%d: part-filled tile %d, room for %ld samples", op.name.c_str(),
              mode, B, q[DAD_FP_REC_PART_TILE], room);
    };
    if (mode == 3) {
        CHECK(ints == DAD_FP_REC_INTS && !r[DAD_FP_SMALL] && r[DAD_FP_FINAL_KERNEL] == DAD_FP_FINAL_NONE && n == (int)ts->dgrads.size(),
              "mode 3 B=%d: %d records for %zu data-gradient launches", B, n, ts->dgrads.size());
        int k = 0;
        for (const BwdStep& s : m.bsteps)
            if (s.kind == BK_DGRAD && k < n) { conv(&r[DAD_FP_HEADER + (size_t)k * ints], s.conv, s.sub, bwd_op(m, s), ts->dgrads[k].g, ts->dgrads[k].ok); ++k; }
        CHECK(k == n, "mode 3 B=%d: %d data-gradient steps, %d records", B, k, n);
        return;
    }
    const Plan& plan = f->train ? m.tplan : m.plan;
    CHECK(f->train == (mode == 2) && r[DAD_FP_FINAL_GX] == (int)f->final_gx && r[DAD_FP_FINAL_GY] == (int)f->final_gy &&
          r[DAD_FP_FINAL_KERNEL] == (f->cc.ok ? DAD_FP_FINAL_CC : DAD_FP_FINAL_POSTERIOR) && (r[DAD_FP_SMALL] != 0) == f->cc.ok,
          "mode %d B=%d: report of the final launch", mode, B);
    if (!f->cc.ok) {
        CHECK(ints == DAD_FP_REC_INTS && n == (int)f->launches.size(), "mode %d B=%d: %d records for %zu launches", mode, B, n, f->launches.size());
        for (int k = 0; k < n && k < (int)f->launches.size(); ++k) {
            const FwdLaunch& l = f->launches[k];
            conv(&r[DAD_FP_HEADER + (size_t)k * ints], l.conv, 0, plan.convs[l.conv], l.g, l.ok);
        }
        return;
    }
    int launched = 0, k = 0;
    for (const CcOp& o : f->cc.ops) launched += o.launched;
    CHECK(ints == DAD_FP_CC_INTS && n == launched && f->launches.empty(), "mode %d B=%d: %d records for %d small-batch launches", mode, B, n, launched);
    for (size_t i = 0; i < f->cc.ops.size() && k < n; ++i) {
        const CcOp& o = f->cc.ops[i];
        if (!o.launched) continue;
        const ConvOp& op = plan.convs[i];
        const int32_t* q = &r[DAD_FP_HEADER + (size_t)k++ * ints];
        CHECK(q[DAD_FP_CC_CONV] == (int)i && q[DAD_FP_CC_TAPS] == op.taps && q[DAD_FP_CC_STRIDE] == op.stride && (q[DAD_FP_CC_WIDE] != 0) == o.wide &&
              (q[DAD_FP_CC_RIDE] != 0) == op.ride && (q[DAD_FP_CC_BIG] != 0) == o.big && (q[DAD_FP_CC_RIDE_IN] != 0) == o.ride_in &&
              q[DAD_FP_CC_TILE_ROWS] == o.tile_rows && (q[DAD_FP_CC_WINDOWED] != 0) == (op.Lout > 32) && q[DAD_FP_CC_SLICE_CH] == o.slice_ch &&
              q[DAD_FP_CC_KSLICES] == o.kslices && q[DAD_FP_CC_NTILES] == o.ntiles && q[DAD_FP_CC_RES_KIND] == o.res_kind,
              "%s B=%d: small-batch report record differs from the launch", op.name.c_str(), B);
        // the instantiation run_conv_cc looks up: conv_ccw by ride_in, conv_cc by big and windowed
        CHECK(small_kernel_exists(op.taps, op.stride, op.ride, o.wide, o.wide ? false : o.big, o.wide ? o.ride_in : false, o.tile_rows, op.Lout > 32),
              "%s B=%d: the report names a small-batch kernel that does not exist", op.name.c_str(), B);
        // ... by the key of its family, as run_conv_cc builds it (a wide launch of a layer longer than 32 positions has none)
        CHECK(o.wide ? !(op.Lout > 32) && family_kernel_exists(FAM_CCW, {op.taps, op.stride, op.ride, o.ride_in, o.tile_rows})
                     : family_kernel_exists(FAM_CC, {op.taps, op.stride, op.ride, o.big, o.tile_rows, op.Lout > 32}),
              "%s B=%d: no kernel of the small-batch family for the launch's key", op.name.c_str(), B);
    }
}

// dad_debug_halo8_plan: one record per conv_halo8_f32 launch of the description, in order, every field recomputed here
// the way the kernel derives it from its ConvParams (conv_halo8.hpp: nchunks, `second`, has_res / has_temb / has_gn,
// lpp and wpp, the tile decode, nvalid of the last tile) — from the ConvOp and LaunchGeom those parameters are filled from.
static long g_halo8_reports = 0, g_halo8_records = 0;
static void check_halo8_report(const HostModel& m, int B, const FwdPlan& f, bool rows) {
    std::vector<int32_t> r;
    halo8_plan_encode(m, f, rows, r);
    CHECK(r.size() >= DAD_H8_HEADER && r[1] == DAD_H8_INTS && r.size() == (size_t)DAD_H8_HEADER + (size_t)r[0] * DAD_H8_INTS, "B=%d: halo8 report of %zu ints",
          B, r.size());
    if (r.size() < DAD_H8_HEADER || r.size() != (size_t)DAD_H8_HEADER + (size_t)r[0] * DAD_H8_INTS) return;
    ++g_halo8_reports;
    int k = 0;
    if (!f.cc.ok && !f.train)
        for (const FwdLaunch& l : f.launches) {
            if (!l.g.halo8) continue;
            CHECK(k < r[0], "B=%d: more halo8 launches than records", B);
            if (k >= r[0]) break;
            const int32_t* q = &r[DAD_H8_HEADER + (size_t)k++ * DAD_H8_INTS];
            const ConvOp& op = m.plan.convs[l.conv];
            const LaunchGeom& g = l.g;
            ++g_halo8_records;
            CHECK(q[DAD_H8_CONV] == l.conv && q[DAD_H8_CFG] == g.cfg && halo8_kernel_exists(g.cfg) && (q[DAD_H8_RIDE] != 0) == g.fused, "%s B=%d: instantiation",
                  op.name.c_str(), B);
            CHECK(family_kernel_exists(FAM_HALO8, {q[DAD_H8_CFG], q[DAD_H8_RIDE]}), "%s B=%d: conv_halo8_f32 (tile %d, ride %d) does not exist", op.name.c_str(), B,
                  q[DAD_H8_CFG], q[DAD_H8_RIDE]);
            const int cin0 = op.cin0, cin1 = op.cin1, KC = 32;
            CHECK((cin0 + cin1) % KC == 0 && cin0 % KC == 0 && q[DAD_H8_CHUNKS] == (cin0 + cin1) / KC, "%s B=%d: %d chunks for %d + %d channels", op.name.c_str(), B,
                  q[DAD_H8_CHUNKS], cin0, cin1);
            int first_second = -1;                          // the first chunk the kernel's `second` is true for
            for (int ch = 0; ch < (cin0 + cin1) / KC; ++ch)
                if (ch * KC >= cin0 && first_second < 0) first_second = ch;
            CHECK((op.src1 >= 0) == (cin1 > 0) && q[DAD_H8_SRC1_CHUNK] == first_second, "%s B=%d: second source from chunk %d, the kernel's %d", op.name.c_str(), B,
                  q[DAD_H8_SRC1_CHUNK], first_second);
            // (the operands as conv_io of dad_lib.hip hands them over: io.res is the trajectory for op.res == -2, a plan buffer for
            // an id >= 0, else null; io.temb exists where op.temb_off >= 0, and io.trow only beside it.  The same expressions as the
            // encoder's: this holds the slots, not the reading of conv_io — keep the two in step with it.)
            CHECK((q[DAD_H8_RES] != 0) == (op.res == -2 || op.res >= 0) && (q[DAD_H8_TEMB] != 0) == (op.temb_off >= 0) &&
                  (q[DAD_H8_PER_ROW] != 0) == (rows && op.temb_off >= 0), "%s B=%d: residual / time embedding", op.name.c_str(), B);
            const bool gn = !op.norm.empty();
            CHECK(g.gn_npt == 0 && (q[DAD_H8_GN] != 0) == gn, "%s B=%d: GroupNorm", op.name.c_str(), B);
            const TileCfg& t = kTiles[g.cfg];
            int wpp = 0;
            if (gn) {
                const int NT = 64 * (t.BM / 32) * 2 * t.SK, F4PL = (64 * t.BM / 4) / NT, cpg = op.cout / 8, cnt4 = 8 * (cpg >> 2);
                const int lpp = cnt4 >> (F4PL == 1 ? 0 : F4PL == 2 ? 1 : F4PL == 4 ? 2 : 3);
                CHECK(NT == g.threads && lpp >= 1 && is_pow2(lpp) && lpp * F4PL == cnt4, "%s B=%d: %d lanes per pair", op.name.c_str(), B, lpp);
                wpp = std::max(1, lpp >> 6);
                CHECK(wpp <= NT / 64 && (NT / 64) % wpp == 0, "%s B=%d: a pair of %d waves in a block of %d", op.name.c_str(), B, wpp, NT / 64);
            }
            CHECK(q[DAD_H8_WPP] == wpp, "%s B=%d: %d waves per pair, the kernel's %d", op.name.c_str(), B, q[DAD_H8_WPP], wpp);
            CHECK(q[DAD_H8_XCD_GN] == g.xcd_gn && q[DAD_H8_MTILES] == g.mtiles && q[DAD_H8_NTILES_N] == g.ntiles_n && g.mtiles * t.BM == op.M, "%s B=%d: grid",
                  op.name.c_str(), B);
            const int last = B - (g.ntiles_n - 1) * 8;      // nvalid of the last N tile
            CHECK(last >= 1 && last <= 8 && (q[DAD_H8_PART_TILE] != 0) == (last < 8), "%s B=%d: last tile holds %d samples", op.name.c_str(), B, last);
        }
    CHECK(k == r[0], "B=%d: %d halo8 launches, %d records", B, k, r[0]);
}

// dad_debug_backward_steps: one record per step of m.bsteps, in order, each field equal to what dad_unet_backward reads for
// that step — the step itself, the forward conv a GroupNorm step belongs to, the geometry `ts` of train_scratch.  The
// derived fields are recomputed here the way the kernels see them (block origins, staged widths), not the way the
// report computes them.
static long g_step_reports = 0;
static void check_backward_steps(const HostModel& m, int B, const TrainScratch& ts, int rc_plan) {
    std::vector<int32_t> r;
    const int rc = backward_steps_report(m, B, r);
    CHECK(rc == rc_plan, "B=%d: the step report returns %d, train_scratch %d", B, rc, rc_plan);
    CHECK(r.size() >= DAD_BS_HEADER && r[DAD_BS_BATCH] == B && r[DAD_BS_RECORD_INTS] == DAD_BS_REC_INTS &&
          r[DAD_BS_STEPS] == (int)m.bsteps.size() && r.size() == DAD_BS_HEADER + m.bsteps.size() * DAD_BS_REC_INTS,
          "B=%d: step report of %zu ints for %zu steps", B, r.size(), m.bsteps.size());
    if (r.size() != DAD_BS_HEADER + m.bsteps.size() * DAD_BS_REC_INTS) return;
    ++g_step_reports;
    const int H = m.cfg.horizon, Hr = m.real_horizon > 0 ? m.real_horizon : H;
    int widest = 0;
    for (const BwdSum& q : m.bsums) widest = std::max(widest, q.C);
    int launches = 0;
    for (size_t at = 0; at < m.bsums.size(); at += dad::COLS_MAX) ++launches;       // the loop of dad_unet_backward
    CHECK(r[DAD_BS_COLSUMS_LAUNCHES] == launches && r[DAD_BS_COLSUMS_ENTRIES] == (int)m.bsums.size() && r[DAD_BS_COLSUMS_WIDEST] == widest,
          "B=%d: column sums: %d launches, %d entries, widest %d", B, r[DAD_BS_COLSUMS_LAUNCHES], r[DAD_BS_COLSUMS_ENTRIES], r[DAD_BS_COLSUMS_WIDEST]);
    CHECK((r[DAD_BS_PADCOPY] != 0) == (Hr != H) && r[DAD_BS_HORIZON] == H && r[DAD_BS_REAL_HORIZON] == Hr && (r[DAD_BS_DX] != 0) == m.bdx,
          "B=%d: padded-horizon copies %d (%d of %d positions)", B, r[DAD_BS_PADCOPY], r[DAD_BS_REAL_HORIZON], r[DAD_BS_HORIZON]);
    size_t nw = 0;
    for (size_t i = 0; i < m.bsteps.size(); ++i) {
        const BwdStep& s = m.bsteps[i];
        const int32_t* q = &r[DAD_BS_HEADER + i * DAD_BS_REC_INTS];
        CHECK(q[DAD_BS_KIND] == (int)s.kind, "B=%d step %zu: kind %d, the plan says %d", B, i, q[DAD_BS_KIND], (int)s.kind);
        int used = 1;                          // fields the kind names; the rest must be 0
        switch (s.kind) {
            case BK_BIAS:
                CHECK(q[DAD_BS_BIAS_ROWS] == s.rows && q[DAD_BS_BIAS_C] == s.C, "B=%d step %zu: bias record", B, i);
                used = 3;
                break;
            case BK_WGRAD: {
                if (nw >= ts.wgrads.size()) { CHECK(false, "B=%d step %zu: no geometry", B, i); break; }
                const WgradShape& sh = ts.wgrads[nw].sh;
                const WgradGeom& g = ts.wgrads[nw++].g;
                const int Ctot = s.C0 + s.C1, WMW = 32 * g.tm, WNW = 32 * g.tn;
                bool inside = false;           // a block whose staged columns [c0, c0 + WNW) hold both sides of the concat
                for (unsigned by = 0; by < g.gy; ++by) inside = inside || (s.C1 > 0 && (int)by * WNW < s.C0 && s.C0 < (int)(by + 1) * WNW);
                int at = 0, fullest = 0, last = 0;
                for (int ks = 0; ks < g.ksplit; ++ks) {
                    const int hi = std::min(sh.B, (ks + 1) * g.sps);
                    last = (hi - at + g.spc - 1) / g.spc;
                    fullest = std::max(fullest, last);
                    at = hi;
                }
                CHECK(q[DAD_BS_WG_TAPS] == s.taps && q[DAD_BS_WG_TILE] == g.tile && (q[DAD_BS_WG_WINDOWED] != 0) == (sh.wshift > 0) &&
                      q[DAD_BS_WG_M] == s.M && q[DAD_BS_WG_C0] == s.C0 && q[DAD_BS_WG_C1] == s.C1 && q[DAD_BS_WG_STRIDE] == s.stride &&
                      q[DAD_BS_WG_PAD] == s.pad && q[DAD_BS_WG_LG] == sh.Lg && q[DAD_BS_WG_LZ] == sh.Lz && q[DAD_BS_WG_GX] == (int)g.gx &&
                      q[DAD_BS_WG_GY] == (int)g.gy, "B=%d step %zu: weight-gradient record (operands)", B, i);
                CHECK((q[DAD_BS_WG_RAGGED] != 0) == (((s.M | s.C0 | s.C1) & 3) != 0) && (q[DAD_BS_WG_CONCAT_INSIDE] != 0) == inside &&
                      (q[DAD_BS_WG_EDGE_M] != 0) == ((int)g.gx * WMW != s.M) && (q[DAD_BS_WG_EDGE_C] != 0) == ((int)g.gy * WNW != Ctot) &&
                      (q[DAD_BS_WG_SWAPPED] != 0) == (s.taps == 4), "B=%d step %zu: weight-gradient record (edges)", B, i);
                CHECK(q[DAD_BS_WG_KSPLIT] == g.ksplit && q[DAD_BS_WG_SLAB_N4] == (g.ksplit > 1 ? (long)s.M * Ctot * s.taps / 4 : 0) &&
                      q[DAD_BS_WG_SAMPLES] == sh.B && q[DAD_BS_WG_SPC] == g.spc && q[DAD_BS_WG_SPS] == g.sps && q[DAD_BS_WG_CHUNKS] == fullest &&
                      q[DAD_BS_WG_LAST_CHUNKS] == last, "B=%d step %zu: weight-gradient record (batch split)", B, i);
                CHECK(std::find(std::begin(kWgradTaps), std::end(kWgradTaps), s.taps) != std::end(kWgradTaps) && g.tile >= 0 && g.tile < 4,
                      "B=%d step %zu: conv_wgrad<%d, tile %d> does not exist", B, i, s.taps, g.tile);
                CHECK(family_kernel_exists(FAM_WGRAD, {q[DAD_BS_WG_TAPS], q[DAD_BS_WG_TILE], q[DAD_BS_WG_WINDOWED]}) &&
                      wgrad_kernel_exists(s.taps, g.tile, sh.wshift > 0), "B=%d step %zu: no conv_wgrad for the step's key (%d, %d, %d)", B, i, s.taps, g.tile,
                      (int)(sh.wshift > 0));
                used = DAD_BS_REC_INTS;
                break;
            }
            case BK_DGRAD:
                CHECK(q[DAD_BS_DG_CONV] == s.conv && q[DAD_BS_DG_SUB] == s.sub && q[DAD_BS_DG_WRITE] == (int)s.write, "B=%d step %zu: data-gradient record", B, i);
                used = 4;
                break;
            case BK_GN: {
                const ConvOp& f = m.tplan.convs[s.conv];
                const int nq = f.cout / 8 / 4;
                CHECK(q[DAD_BS_GN_NV] == s.nv && q[DAD_BS_GN_CPG] == f.cout / 8 && q[DAD_BS_GN_L] == f.Lout && q[DAD_BS_GN_LREAL] == f.lreal &&
                      q[DAD_BS_GN_CPG_REAL] == f.gn_real && (q[DAD_BS_GN_DTEMB] != 0) == (f.temb_off >= 0) && q[DAD_BS_GN_C] == f.cout &&
                      (q[DAD_BS_GN_SHORT_PAIR] != 0) == (nq * f.Lout < 64), "B=%d step %zu (%s): GroupNorm record", B, i, f.name.c_str());
                // the wave form holds a pair in nv x 64 float4; the block form needs a power-of-two quad count <= 64
                CHECK(s.nv == 0 ? (nq >= 1 && nq <= 64 && is_pow2(nq)) : (nq * f.Lout <= s.nv * 64 && is_pow2(nq) && nq <= 64),
                      "B=%d step %zu (%s): a pair of %d float4 on gn_mish_bwd_wave_kernel<%d>", B, i, f.name.c_str(), nq * f.Lout, s.nv);
                used = 9;
                break;
            }
            case BK_RESID:
                CHECK(q[DAD_BS_RS_WRITE] == (int)s.write && q[DAD_BS_RS_N] == std::min<long>(s.n, INT32_MAX) && (q[DAD_BS_RS_TO_X] != 0) == (s.out.sp == BSP_DX),
                      "B=%d step %zu: residual record", B, i);
                used = 4;
                break;
            case BK_COLS:
                CHECK(q[DAD_BS_CL_C] == s.C && q[DAD_BS_CL_OFF] == s.off && q[DAD_BS_CL_LD] == s.ld && q[DAD_BS_CL_ROWS] == s.rows &&
                      q[DAD_BS_CL_WRITE] == (int)s.write, "B=%d step %zu: column-take record", B, i);
                CHECK(s.C % 4 == 0 && s.off % 4 == 0 && s.ld % 4 == 0 && s.off + s.C <= s.ld, "B=%d step %zu: take_cols of %d columns at %d of %d", B, i, s.C, s.off, s.ld);
                used = 6;
                break;
        }
        for (int k = used; k < DAD_BS_REC_INTS; ++k) CHECK(q[k] == 0, "B=%d step %zu: field %d of a kind-%d record is %d", B, i, k, (int)s.kind, q[k]);
    }
    CHECK(nw == ts.wgrads.size(), "B=%d: %zu weight-gradient geometries for %zu steps", B, ts.wgrads.size(), nw);
}

static void check_arch(const Arch& a, int precision) {
    HostModel m;
    dad_cfg& c = m.cfg;
    c.transition_dim = a.td; c.dim = a.dim; c.time_dim = a.time_dim;
    c.n_levels = (int)a.mults.size();
    for (size_t i = 0; i < a.mults.size(); ++i) c.channels[i] = a.dim * a.mults[i];
    c.kernel_size = a.ks; c.horizon = a.horizon; c.n_timesteps = 20;
    c.predict_epsilon = c.clip_denoised = 1;
    m.precision = precision;               // (build_plan decides the kernel families from it)
    int rc = check_cfg(&c);
    if (rc != DAD_OK) { printf("  %-14s refused: %s\n", a.name, g_err); return; }
    for (size_t i = 0; i < a.real.size(); ++i) m.real_channels[i] = a.real[i];
    m.real_horizon = a.hreal;
    rc = build_plan(&m);
    if (rc != DAD_OK) { printf("  %-14s refused: %s\n", a.name, g_err); return; }
    if (a.hreal > 0) {
        int masked = 0;
        for (const ConvOp& op : m.plan.convs) {
            const int rows = op.kind == CONV_DOWN ? op.Lout : op.Lin;        // GEMM rows per sample
            CHECK(op.lreal >= 0 && op.lreal < rows + 1, "%s: lreal %d of %d", op.name.c_str(), op.lreal, rows);
            if (op.lreal > 0) ++masked;
            if (op.src0 == -2) CHECK(op.src_len == a.hreal, "%s: external rows %d", op.name.c_str(), op.src_len);
            else CHECK(op.src_len == 0, "%s: src_len on an internal tensor", op.name.c_str());
        }
        CHECK(masked == (int)m.plan.convs.size(), "%d of %zu convs know their real length", masked, m.plan.convs.size());
        CHECK(!cc_plan(m, 1).ok, "padded horizon took the small-batch kernels");
    }
    if (!a.real.empty()) {
        int padded_ops = 0;
        for (const ConvOp& op : m.plan.convs) {
            if (op.gn_real > 0) { ++padded_ops; CHECK(!op.norm.empty() && op.gn_real < op.cout / 8, "%s: gn_real %d of %d", op.name.c_str(), op.gn_real, op.cout / 8); }
        }
        CHECK(padded_ops > 0, "no conv knows its real group width");
        // (padded groups train: the training plan's convs know the real group width as well — the GroupNorm
        // backward divides its pair means by it)
        for (size_t i = 0; i < m.tplan.convs.size() && i < m.plan.convs.size(); ++i)
            CHECK(m.tplan.convs[i].gn_real == m.plan.convs[i].gn_real, "%s: training plan lost gn_real", m.plan.convs[i].name.c_str());
        CHECK(!cc_plan(m, 1).ok, "padded groups took the small-batch kernels");
    }
    const Plan& P = m.plan;
    CHECK(P.final_act >= 0 && P.final_act < (int)P.bufs.size(), "final_act %d", P.final_act);

    // buffers are disjoint and inside floats_per_sample
    for (size_t i = 0; i < P.bufs.size(); ++i) {
        CHECK(P.bufs[i].offset % 4 == 0, "buffer %zu offset %ld not float4 aligned", i, P.bufs[i].offset);
        CHECK(P.bufs[i].offset + P.bufs[i].per_sample <= P.floats_per_sample, "buffer %zu overruns", i);
        for (size_t j = i + 1; j < P.bufs.size(); ++j) {
            const bool apart = P.bufs[i].offset + P.bufs[i].per_sample <= P.bufs[j].offset ||
                               P.bufs[j].offset + P.bufs[j].per_sample <= P.bufs[i].offset;
            CHECK(apart, "buffers %zu and %zu overlap", i, j);
        }
    }
    // every op reads / writes buffers big enough for it, and never its own output
    double flops = 0;
    int temb_seen = 0;
    for (const ConvOp& op : P.convs) {
        auto cap = [&](int id) { return id >= 0 ? P.bufs[id].per_sample : 0L; };
        const long out_elems = (long)op.cout * (op.kind == CONV_UP ? 2 * op.Lin : op.Lout);
        CHECK(op.dst >= 0 && cap(op.dst) >= out_elems, "%s: dst too small", op.name.c_str());
        if (op.src0 >= 0) CHECK(cap(op.src0) >= (long)op.cin0 * op.Lin, "%s: src0 too small", op.name.c_str());
        if (op.src1 >= 0) CHECK(cap(op.src1) >= (long)op.cin1 * op.Lin, "%s: src1 too small", op.name.c_str());
        CHECK(op.dst != op.src0 && op.dst != op.src1, "%s: in-place conv", op.name.c_str());
        if (op.res >= 0) CHECK(op.res != op.dst && cap(op.res) >= out_elems, "%s: residual buffer", op.name.c_str());
        if (op.rdst >= 0) CHECK(op.rdst != op.dst && op.rdst != op.src0 && op.rdst != op.src1 &&
                                cap(op.rdst) >= out_elems, "%s: ride buffer", op.name.c_str());
        if (op.rider_of >= 0)
            CHECK(op.rider_of < (int)P.convs.size() && P.convs[op.rider_of].rdst == op.dst &&
                  P.convs[op.rider_of].rname == op.name, "%s: rider link", op.name.c_str());
        CHECK(op.cin_pad >= op.cin0 + op.cin1, "%s: cin_pad", op.name.c_str());
        if (op.temb_off >= 0) {
            CHECK(op.temb_off + op.cout <= P.temb_width, "%s: time table slice", op.name.c_str());
            temb_seen += op.cout;
        }
        flops += op.flops_per_sample;
    }
    CHECK(temb_seen == P.temb_width, "time table width %d vs %d", temb_seen, P.temb_width);
    CHECK(flops > 0, "flops");

    // weights: load synthetic tensors for every expected key, then pack every op
    if (a.pack) {
        uint64_t st = 12345;
        for (const auto& kv : m.expected) {
            HostTensor& t = m.raw[kv.first];
            t.shape = kv.second;
            size_t n = 1;
            for (int64_t d : kv.second) n *= (size_t)d;
            t.data.resize(n);
            for (float& v : t.data) v = synth(st) * 0.05f;
        }
        // the weight table as dad_model_finalize walks it (data-gradient images where the net trains)
        m.training = precision == DAD_PREC_FP32 && training_refusal(m) == nullptr;
        const std::vector<WeightEntry> table = weight_table(m);
        size_t arena = 0;
        std::vector<float> img, want;
        for (const WeightEntry& e : table) {
            rc = pack_entry(&m, e, img);
            CHECK(rc == DAD_OK, "%s: pack_entry: %s", e.key.c_str(), g_err);
            if (rc != DAD_OK) continue;
            CHECK(img.size() == e.size(), "%s: %zu floats packed, the table says %zu", e.key.c_str(), img.size(), e.size());
            arena += (img.size() * sizeof(float) + 255) / 256 * 256;
            const std::vector<float>& src = m.raw[e.key].data;
            if (e.img.n == 0) {          // a copy: the tensor, `reps` times
                CHECK((size_t)e.floats == src.size(), "%s: copy of %ld floats", e.key.c_str(), e.floats);
                for (int r = 0; r < e.reps; ++r)
                    CHECK(std::equal(src.begin(), src.end(), img.begin() + r * src.size()), "%s: copy %d", e.key.c_str(), r);
                if (e.to == WT_BIAS || e.to == WT_RBIAS)
                    CHECK(img.size() == (size_t)m.plan.convs[e.conv].M, "%s: bias size", e.key.c_str());
                continue;
            }
            const ConvOp& op = e.to == WT_W ? m.plan.convs[e.conv] : e.to == WT_BWD_W ? m.bconvs[e.conv].op[e.sub] : m.bfinal;
            CHECK(img.size() == (size_t)op.cin_pad * op.wtaps() * op.M, "%s: packed size", op.name.c_str());
            if (op.x3) CHECK(op.c1 > 0 && op.c2 > 0 && std::isfinite(op.c1), "%s: split scales", op.name.c_str());
            // the explicit loops; a split-f16 image is compared after the same split of theirs
            want = e.to == WT_W ? ref_fwd_image(m, op) : e.to == WT_BWD_W ? ref_bwd_image(m, m.tplan.convs[e.conv], m.bconvs[e.conv], e.sub)
                                                     : ref_bfinal_image(m);
            if (op.x3) split_f16_image(want);
            CHECK(want.size() == img.size() && std::memcmp(want.data(), img.data(), img.size() * sizeof(float)) == 0,
                  "%s: image differs from the explicit packing loops", op.name.c_str());
            // the image of one source tensor is a permutation of it plus zero padding
            const bool one_source = e.to == WT_W ? !op.x3 : e.to == WT_BWD_W && m.bconvs[e.conv].n == 1;
            if (one_source) {
                double s_in = 0, s_out = 0;
                for (float v : src) s_in += v;
                if (!e.key2.empty()) for (float v : m.raw[e.key2].data) s_in += v;
                for (float v : img) s_out += v;
                const double tol = e.to == WT_W ? 1e-6 : 1e-5;
                CHECK(std::fabs(s_in - s_out) <= tol * (1 + std::fabs(s_in)), "%s: packed checksum", op.name.c_str());
            }
        }
        CHECK(arena <= arena_bytes_needed(m, table), "arena estimate %zu < %zu", arena_bytes_needed(m, table), arena);
    }

    // what the kernels assume of an accepted launch (`floats_per_sample`: activations in front of the split-K slabs,
    // `ws`: bytes the size query reports for the batch)
    auto check_geom = [&](const ConvOp& op, const LaunchGeom& g, int B, long floats_per_sample, size_t ws) {
            const TileCfg& t = kTiles[g.cfg];
            CHECK(tile_valid(op, g.cfg), "%s: invalid tile %d", op.name.c_str(), g.cfg);
            CHECK(g.threads == 64 * (t.BM / 32) * (t.BN / 32) * t.SK && g.threads <= 1024, "threads %d", g.threads);
            CHECK(g.lds_bytes <= dad::kLdsBytes, "%s: LDS %zu", op.name.c_str(), g.lds_bytes);
            CHECK(g.kc % (op.x3 ? 16 : 8) == 0 && (g.kc / (op.x3 ? 16 : 8)) % t.SK == 0, "%s: K chunk %d", op.name.c_str(), g.kc);
            const long tiles = (long)g.mtiles * g.ntiles_n;
            CHECK((long)g.gx * g.gy * g.gz == tiles * g.split.kslices, "%s: grid %u %u %u vs %ld tiles x %d",
                  op.name.c_str(), g.gx, g.gy, g.gz, tiles, g.split.kslices);
            CHECK(g.gy <= 65535 && g.gz <= 65535, "grid dims");
            CHECK(g.ntiles_n * (t.BN / op.Lout) >= B, "%s: N tiles do not cover the batch", op.name.c_str());
            if (g.split.kslices > 1) {
                CHECK(tiles <= kMaxSplitTiles, "ticket table");
                CHECK(!g.fused, "%s: ride under grid split-K", op.name.c_str());
                const int nchunks = (op.cin0 + op.cin1 + g.kc - 1) / g.kc;
                CHECK((g.split.kslices - 1) * g.split.chunks_per_slice < nchunks &&
                      g.split.kslices * g.split.chunks_per_slice >= nchunks, "%s: K slices", op.name.c_str());
                const size_t slab_end = ((size_t)floats_per_sample * B + (size_t)g.split.slab_floats) * sizeof(float);
                CHECK(slab_end <= ws, "%s B=%d: slab beyond the workspace", op.name.c_str(), B);
            }
            if (g.xcd_gn > 0) {
                const int gm = 8 / g.xcd_gn;
                CHECK(g.mtiles % gm == 0 && g.ntiles_n % g.xcd_gn == 0 && (1 << g.xcd_mts) == g.mtiles / gm &&
                      g.xcd_ntn == g.ntiles_n / g.xcd_gn, "%s: XCD order", op.name.c_str());
                // the kernel's decode of a linear block id must be a bijection onto tiles
                std::vector<char> hit((size_t)tiles, 0);
                for (long wg = 0; wg < tiles; ++wg) {
                    const int cc = (int)(wg & 7), j = (int)(wg >> 3);
                    const int im = cc / g.xcd_gn, in = cc - im * g.xcd_gn;
                    const int mt = (im << g.xcd_mts) + (j & ((1 << g.xcd_mts) - 1));
                    const int nt = in * g.xcd_ntn + (j >> g.xcd_mts);
                    CHECK(mt < g.mtiles && nt < g.ntiles_n, "%s: XCD decode out of range", op.name.c_str());
                    if (mt < g.mtiles && nt < g.ntiles_n) hit[(size_t)mt * g.ntiles_n + nt]++;
                }
                for (char h : hit) CHECK(h == 1, "%s: XCD decode not a bijection", op.name.c_str());
            }
            if (g.xswz != 0) {
                const int pad = op.taps / 2, kp4 = (g.kc + 4) / 4;
                CHECK(xswz_conflict_free(g.xswz, op.Lout, op.stride, pad, kp4, t.BN), "%s: slot shifts conflict", op.name.c_str());
                const int S = t.BN / op.Lout;
                for (int s = 0; s + 1 < S; ++s) {
                    const int d0 = (int)((g.xswz >> (4 * s)) & 15), d1 = (int)((g.xswz >> (4 * (s + 1))) & 15);
                    CHECK(d0 - d1 <= pad * kp4, "%s: shift pushes a sample onto its neighbour", op.name.c_str());
                }
                // the stage was sized with kXSwzPad floats of slack for shifts of at most 15 slots
                CHECK(15 * 4 <= dad::kXSwzPad, "slot shift slack");
            }
            if (g.fused) CHECK(op.ride && op.kind == CONV_K5 && (op.taps & 1) && op.stride == 1 && !op.x3 && !op.bdir, "%s: ride", op.name.c_str());
    };
    // launches: every batch size, every forced tile, with and without split-K / fusion
    const int batches[] = {1, 2, 3, 5, 8, 13, 31, 33, 64, 100, 128, 256, 257, 1024, 2048};
    long launches = 0;
    for (int force = -1; force < kNumTiles; ++force)
        for (int variant = 0; variant < 3; ++variant) {
            m.force_tile = force;
            m.split_enabled = variant != 1;
            m.fuse_residual = variant != 2;
            for (int B : batches) {
                const size_t ws = workspace_bytes(m, B);
                for (const ConvOp& op : m.plan.convs) {
                    LaunchGeom g;
                    rc = plan_launch(m, op, B, g);
                    if (rc != DAD_OK) {
                        // a refusal must be a message, never a crash; the heuristic (force = -1) must
                        // always find a launch for an architecture check_cfg accepted
                        CHECK(force >= 0, "%s B=%d: %s", op.name.c_str(), B, g_err);
                        continue;
                    }
                    ++launches;
                    check_geom(op, g, B, P.floats_per_sample, ws);
                }
                // the forward description the entry points replay (plan_forward): the plan's convs minus exactly the
                // riders whose carrier is fused, every accepted geometry as checked above, a GroupNorm pass where the
                // launch is windowed and normalised and nowhere else, the slabs inside the size the query reports
                FwdPlan f;
                rc = plan_forward(m, false, B, false, f);
                CHECK(rc == DAD_OK || force >= 0, "B=%d: %s", B, g_err);
                CHECK(f.bytes == ws && !f.cc.ok && !f.train && f.batch == B, "B=%d: description of another call (%zu bytes, the query says %zu)", B, f.bytes, ws);
                check_forward_report(m, 1, B, &f, nullptr, rc);
                if (rc == DAD_OK) check_halo8_report(m, B, f, true);
                {   // ... and of the shared-timestep call, which may take the small-batch kernels
                    FwdPlan f0;
                    const int rc0 = plan_forward(m, false, B, true, f0);
                    check_forward_report(m, 0, B, &f0, nullptr, rc0);
                    if (rc0 == DAD_OK) check_halo8_report(m, B, f0, false);
                }
                CHECK(workspace_bytes(m, B) == ws, "B=%d: the size query depends on who asks", B);
                std::vector<int> at(P.convs.size(), -1);         // conv -> its place in the list
                bool all_ok = true;
                for (size_t k = 0; k < f.launches.size(); ++k) {
                    const FwdLaunch& l = f.launches[k];
                    CHECK(l.conv >= 0 && l.conv < (int)P.convs.size() && (k == 0 || l.conv > f.launches[k - 1].conv), "B=%d: launch %zu is conv %d", B, k, l.conv);
                    if (l.conv < 0 || l.conv >= (int)P.convs.size()) continue;
                    at[l.conv] = (int)k;
                    const ConvOp& op = P.convs[l.conv];
                    LaunchGeom g;
                    CHECK((plan_launch(m, op, B, g) == DAD_OK) == l.ok, "%s B=%d: the description disagrees with plan_launch", op.name.c_str(), B);
                    all_ok = all_ok && l.ok;
                    if (l.ok) {
                        check_geom(op, l.g, B, P.floats_per_sample, ws);
                        const bool pass = l.g.windowed && !op.norm.empty();
                        CHECK((l.g.gn_npt > 0) == pass, "%s B=%d: GroupNorm pass %d on a %s launch", op.name.c_str(), B, l.g.gn_npt, pass ? "windowed, normalised" : "plain");
                        if (pass) {
                            const long pair = (long)(op.cout / 8) * op.Lout, per = dad::GNP_THREADS * 4L;
                            CHECK((l.g.gn_npt & (l.g.gn_npt - 1)) == 0 && l.g.gn_npt <= dad::kGnPassMaxNpt && pair <= l.g.gn_npt * per &&
                                  (l.g.gn_npt == 1 || pair > l.g.gn_npt / 2 * per) && (op.cout / 8) % 4 == 0,
                                  "%s B=%d: gn_pass_kernel<%d> for pairs of %ld elements", op.name.c_str(), B, l.g.gn_npt, pair);
                        }
                    }
                    // (refused or not: its slab is inside the reported size)
                    CHECK(((size_t)P.floats_per_sample * B + (size_t)l.g.split.slab_floats) * sizeof(float) <= ws, "%s B=%d: slab beyond the workspace", op.name.c_str(), B);
                }
                CHECK((rc == DAD_OK) == all_ok, "B=%d: the description's refusal is not that of its launches", B);
                for (size_t i = 0; i < P.convs.size(); ++i) {
                    const ConvOp& op = P.convs[i];
                    const bool rides = op.rider_of >= 0 && at[op.rider_of] >= 0 && f.launches[at[op.rider_of]].g.fused;
                    CHECK((at[i] < 0) == rides, "%s B=%d: %s, its carrier is %sfused", op.name.c_str(), B, at[i] < 0 ? "not listed" : "listed", rides ? "" : "not ");
                    if (at[i] >= 0 && f.launches[at[i]].g.fused)
                        CHECK(i + 1 < P.convs.size() && P.convs[i + 1].rider_of == (int)i, "%s B=%d: fused without a rider", op.name.c_str(), B);
                }
                CHECK(f.final_lds <= dad::kLdsBytes && f.final_gx >= 1 && f.final_gy >= 1 && f.final_gy <= 65535 &&
                      (long)f.final_gx * dad::FINAL_COLS >= (long)B * traj_horizon(m), "B=%d: final launch %u x %u, %zu bytes", B, f.final_gx, f.final_gy, f.final_lds);
            }
        }
    // small-batch (consumer-combine) plans: slabs disjoint and inside the workspace, inputs finished
    // before they are read finished, slices whole groups, every launch fits LDS
    m.force_tile = -1; m.split_enabled = true; m.fuse_residual = true;
    long cc_plans = 0;
    for (int B : {1, 2, 3, 5, 8, 13, 16, 33}) {
        const CcPlan cc = cc_plan(m, B);
        if (!cc.ok) continue;
        ++cc_plans;
        CHECK(precision == DAD_PREC_FP32 && (long)B * c.horizon <= m.cc_max_rows, "CC plan outside its domain");
        CHECK(workspace_bytes(m, B) >= ((size_t)P.floats_per_sample * B + (size_t)cc.slab_floats) * sizeof(float), "CC workspace");
        {   // the description of a call that takes these kernels holds this plan and no conv-GEMM launch
            FwdPlan f;
            CHECK(plan_forward(m, false, B, true, f) == DAD_OK && f.cc.ok && f.launches.empty() && f.bytes == workspace_bytes(m, B) &&
                  f.cc.slab_floats == cc.slab_floats && f.final_gx == (unsigned)B && f.final_lds <= dad::kLdsBytes, "B=%d: small-batch description", B);
            check_forward_report(m, 0, B, &f, nullptr, DAD_OK);
        }
        std::vector<std::pair<long, long>> spans;
        std::vector<char> finished(P.convs.size(), 0);
        for (size_t i = 0; i < P.convs.size(); ++i) {
            const ConvOp& op = P.convs[i];
            const CcOp& o = cc.ops[i];
            if (!o.launched) { CHECK(op.rider_of >= 0 && P.convs[op.rider_of].ride, "%s not launched", op.name.c_str()); continue; }
            CHECK(o.kslices >= 1 && o.kslices <= (o.wide ? kCcwMaxSlabs : kCcMaxSlabs) && o.slice_ch % 32 == 0 &&
                  (o.wide || o.slice_ch <= kCcMaxSlice),
                  "%s: slices %d x %d", op.name.c_str(), o.kslices, o.slice_ch);
            CHECK((long)o.kslices * o.slice_ch >= op.cin0 + op.cin1 && (long)o.kslices * o.slice_ch <= op.cin_pad,
                  "%s: slices do not cover the input channels", op.name.c_str());
            CHECK(op.cin1 == 0 || op.cin0 % o.slice_ch == 0, "%s: slice straddles the concat", op.name.c_str());
            CHECK(o.lds_bytes <= dad::kLdsBytes, "%s: CC LDS %zu", op.name.c_str(), o.lds_bytes);
            if (o.wide) {
                // conv_ccw.hpp's contract: 16-channel granules, channel counts in float4, LDS sized by its formula
                CHECK((op.kc == 16 || op.bdir) && op.cin0 % 4 == 0 && op.cin1 % 4 == 0 && op.src0 != -2,
                      "%s: wide conv on an input it cannot stage", op.name.c_str());
                CHECK(o.lds_bytes == dad::ccw_lds_floats(o.slice_ch, op.taps, op.Lin, op.Lout, o.tile_rows) * sizeof(float),
                      "%s: wide LDS size", op.name.c_str());
            } else {
                CHECK(op.kind != CONV_1X1, "%s: conv_cc has no 1x1 form", op.name.c_str());
                CHECK((size_t)(o.slice_ch / 16) * op.wtaps() * 128 <= (size_t)6 * 512, "%s: weight staging registers", op.name.c_str());
                CHECK(o.kslices <= 8 || o.slice_ch == kCcMaxSlice, "%s: more than 8 slabs below the widest slice", op.name.c_str());
            }
            if (op.Lout > 32) {           // windowed tiles: 32 rows of one sample each, stride-1 k-tap convs of conv_cc only
                CHECK(!o.wide && op.kind == CONV_K5 && op.stride == 1 && o.tile_rows == 32 && op.Lout % 32 == 0 &&
                      o.ntiles == B * (op.Lout / 32), "%s: windowed tiles", op.name.c_str());
                CHECK(o.lds_bytes >= ((size_t)(32 + 2 * (op.taps / 2)) * (o.slice_ch + 4) + (size_t)op.wtaps() * 32 * (o.slice_ch + 4)) * sizeof(float),
                      "%s: windowed LDS", op.name.c_str());
            } else {
                CHECK((o.tile_rows == 16 || o.tile_rows == 32) && o.tile_rows % op.Lout == 0 &&
                      o.ntiles * (o.tile_rows / op.Lout) >= B, "%s: tiles do not cover the batch", op.name.c_str());
            }
            if (o.wide) CHECK(op.Lin <= 32 && op.Lout <= 32, "%s: conv_ccw beyond 32 positions", op.name.c_str());
            const long n = (long)o.kslices * o.out_rows * o.out_cols;
            spans.push_back({o.oslab, o.oslab + n});
            if (o.orslab >= 0) spans.push_back({o.orslab, o.orslab + n});
            CHECK((o.orslab >= 0) == op.ride, "%s: ride slab", op.name.c_str());
            for (const CcInput* in : {&o.in0, &o.in1}) {
                if (in->kind == 3) {
                    CHECK(in->producer >= 0 && in->producer < (int)i && cc.ops[in->producer].launched && !finished[in->producer],
                          "%s: reads %d in pieces twice", op.name.c_str(), in->producer);
                    finished[in->producer] = 1;
                    const ConvOp& q = P.convs[in->producer];
                    if (!q.norm.empty()) CHECK(o.slice_ch % (q.cout / 8) == 0, "%s: slice splits a GroupNorm group", op.name.c_str());
                    const CcOp& qo = cc.ops[in->producer];
                    if (qo.res_kind == 3) CHECK(cc.ops[qo.res_ride].orslab >= 0 && qo.res_ride < in->producer, "%s: ride source", op.name.c_str());
                    if (qo.res_kind == 4) CHECK(cc.ops[qo.res_ride].launched && P.convs[qo.res_ride].kind == CONV_1X1 && qo.res_ride < in->producer,
                                                "%s: residual conv source", op.name.c_str());
                    const long pair = q.norm.empty() ? 0 : (long)(q.cout / 8) * op.Lin;
                    const int spt = op.Lout > 32 ? 1 : o.tile_rows / op.Lout;
                    if (o.wide) {
                        CHECK(qo.kslices <= kCcwMaxSlabs && (qo.res_kind < 3 || cc.ops[qo.res_ride].kslices <= kCcwMaxSlabs),
                              "%s: wide conv fed more than %d slabs", op.name.c_str(), kCcwMaxSlabs);
                        CHECK(pair <= kCcwMaxPair, "%s: pair of %ld elements", op.name.c_str(), pair);
                        if (!q.norm.empty()) CHECK((long)spt * (o.slice_ch / (q.cout / 8)) <= kCcwMaxPairs, "%s: pairs per block", op.name.c_str());
                    } else {
                        CHECK(pair <= 1024, "%s: conv_cc normalises at most 1024 elements per pair (%ld)", op.name.c_str(), pair);
                    }
                }
            }
        }
        CHECK(cc.final_producer >= 0 && !finished[cc.final_producer], "final conv output already finished");
        if (cc.final_producer >= 0) {
            const ConvOp& f = P.convs[cc.final_producer];
            CHECK((long)(f.cout / 8) * f.Lout <= 1024, "final_cc normalises at most 1024 elements per pair");
        }
        std::sort(spans.begin(), spans.end());
        for (size_t k = 0; k + 1 < spans.size(); ++k) CHECK(spans[k].second <= spans[k + 1].first, "CC slabs overlap");
        if (!spans.empty()) CHECK(spans.front().first >= 0 && spans.back().second <= cc.slab_floats, "CC slabs outside their region");
    }
    // training plan + backward plan (fp32): every tensor of the forward owns its buffer, the data-gradient
    // launches find a tile at every batch, their packed images are permutations of the weights, and the flat
    // gradient buffer holds every conv / GroupNorm / final-conv tensor exactly once
    long bwd_launches = 0;
    if (precision == DAD_PREC_FP32 && training_refusal(m) == nullptr) {
        const Plan& T = m.tplan;
        CHECK(T.convs.size() == P.convs.size() && m.bconvs.size() == T.convs.size(), "training plan size");
        std::vector<int> writers(T.bufs.size(), 0);
        for (const ConvOp& op : T.convs) {
            ++writers[op.dst];
            CHECK(op.norm.empty() == (op.pre < 0) && (op.pre < 0) == (op.stats < 0), "%s: pre / stats buffers", op.name.c_str());
            if (op.pre >= 0) {
                ++writers[op.pre]; ++writers[op.stats];
                CHECK(T.bufs[op.pre].per_sample >= (long)op.cout * op.Lout && T.bufs[op.stats].per_sample >= 16, "%s: pre / stats size", op.name.c_str());
            }
        }
        for (size_t i = 0; i < writers.size(); ++i) CHECK(writers[i] <= 1, "training buffer %zu written by %d launches", i, writers[i]);
        for (size_t i = 0; i < T.bufs.size(); ++i) CHECK(T.bufs[i].offset + T.bufs[i].per_sample <= T.floats_per_sample, "training buffer %zu overruns", i);
        std::map<std::string, int> seen;
        long end = 0;
        for (const auto& gs : m.grad_slots) {
            ++seen[gs.key];
            CHECK(gs.offset >= end && gs.offset % 4 == 0, "gradient slot %s overlaps", gs.key.c_str());
            end = gs.offset + gs.numel;
            auto ex = m.expected.find(gs.key);
            CHECK(ex != m.expected.end(), "gradient slot %s is not a parameter", gs.key.c_str());
            if (ex != m.expected.end()) {
                long n = 1;
                for (int64_t d : ex->second) n *= (long)d;
                CHECK(n == gs.numel, "gradient slot %s: %ld elements, parameter has %ld", gs.key.c_str(), gs.numel, n);
            }
        }
        CHECK(end <= m.grad_numel, "gradient buffer too short");
        for (const auto& kv : m.expected)
            if (kv.first.find("time_mlp.") == std::string::npos) CHECK(seen[kv.first] == 1, "parameter %s has %d gradient slots", kv.first.c_str(), seen[kv.first]);
        for (size_t i = 0; i < T.convs.size(); ++i) {
            const ConvOp& f = T.convs[i];
            const HostModel::BwdConv& b = m.bconvs[i];
            CHECK(b.n == (f.cin1 > 0 ? 2 : 1), "%s: %d data-gradient launches", f.name.c_str(), b.n);
            int covered = 0;
            for (int k = 0; k < b.n; ++k) {
                covered += b.c_n[k];
                CHECK(b.op[k].cout >= b.c_n[k] && b.op[k].cout % 32 == 0 && b.op[k].cin0 == f.cout, "%s: data-gradient shape", f.name.c_str());
                for (int B : {1, 3, 9, 32, 256}) {
                    LaunchGeom g;
                    rc = plan_launch(m, b.op[k], B, g);
                    CHECK(rc == DAD_OK, "%s B=%d: %s", b.op[k].name.c_str(), B, g_err);
                    if (rc == DAD_OK) { ++bwd_launches; CHECK(g.lds_bytes <= dad::kLdsBytes && !g.fused, "%s: geometry", b.op[k].name.c_str()); }
                }
            }
            CHECK(covered == f.cin0 + f.cin1, "%s: data gradients cover %d of %d input channels", f.name.c_str(), covered, f.cin0 + f.cin1);
        }
        for (int B : {1, 9, 256}) {
            LaunchGeom g;
            rc = plan_launch(m, m.bfinal, B, g);
            CHECK(rc == DAD_OK, "final data gradient B=%d: %s", B, g_err);
        }
        // the backward plan's steps (dad_unet_backward replays them): a gradient is read only after a step wrote it,
        // its first write overwrites and later ones add; every gradient slot is written by exactly one weight-gradient
        // step or one column sum; the partial sums tile their region; a gradient reaches the trajectory
        CHECK(m.bwd_rc == DAD_OK, "backward plan: %s", m.bwd_err.c_str());
        CHECK(m.bdx, "backward plan: no gradient reaches the trajectory");
        std::vector<char> gwritten(T.bufs.size(), 0);
        char dxwritten = 0;
        std::vector<int> slot_writes(m.grad_slots.size(), 0);
        std::vector<std::pair<long, long>> parts;      // [first, end) partial-sum rows of a step, units of B floats
        for (const BwdStep& s : m.bsteps) {
            for (const BwdRef* r : {&s.in, &s.z0, &s.z1}) {
                CHECK(r->sp != BSP_DX, "a step reads d x");
                if (r->sp == BSP_GRAD) CHECK(gwritten[r->buf], "a step reads the gradient of buffer %d before it is written", r->buf);
            }
            if (s.kind == BK_WGRAD) {
                ++slot_writes[s.slot];
                CHECK(s.out.sp == BSP_NONE && m.grad_slots[s.slot].numel == (long)s.M * (s.C0 + s.C1) * s.taps,
                      "weight gradient of %s: shape", m.grad_slots[s.slot].key.c_str());
            } else if (s.kind == BK_BIAS) {
                CHECK(s.out.sp == BSP_NONE, "bias step writes a tensor");
                parts.push_back({s.part, s.part + round_up(s.C, 4)});
            } else {
                CHECK(s.out.sp == BSP_GRAD || s.out.sp == BSP_DX, "step kind %d writes no gradient", (int)s.kind);
                char& w = s.out.sp == BSP_DX ? dxwritten : gwritten[s.out.buf];
                CHECK((s.write == BW_SET) == !w, "step kind %d: first write overwrites, later ones accumulate", (int)s.kind);
                CHECK(s.write != BW_STAGE || (s.kind == BK_DGRAD && bwd_op(m, s).kind == CONV_UP), "staged write of a non-CONV_UP step");
                w = 1;
                if (s.kind == BK_GN) parts.push_back({s.part, s.part + 3L * round_up(T.convs[s.conv].cout, 4)});
            }
        }
        for (const BwdSum& q : m.bsums) {
            ++slot_writes[q.slot];
            CHECK(m.grad_slots[q.slot].numel == q.C, "column sum into %s: %d columns", m.grad_slots[q.slot].key.c_str(), q.C);
            bool inside = false;
            for (const auto& r : parts) inside = inside || (q.part >= r.first && q.part + q.C <= r.second);
            CHECK(inside, "column sum into %s reads outside the partial sums of a step", m.grad_slots[q.slot].key.c_str());
        }
        for (size_t k = 0; k < slot_writes.size(); ++k)
            CHECK(slot_writes[k] == 1, "gradient slot %s written %d times", m.grad_slots[k].key.c_str(), slot_writes[k]);
        std::sort(parts.begin(), parts.end());
        long part_end = 0;
        for (const auto& r : parts) { CHECK(r.first == part_end, "partial sums: gap or overlap at %ld", r.first); part_end = r.second; }
        CHECK(part_end == m.bpart, "partial sums: %ld rows, the plan counts %ld", part_end, m.bpart);
        for (int B : {1, 3, 9, 32, 128, 250, 256, 512}) {
            TrainScratch ts;
            rc = train_scratch(m, B, ts);
            CHECK(rc == DAD_OK, "backward geometry B=%d: %s", B, g_err);
            check_forward_report(m, 3, B, nullptr, &ts, rc);
            check_backward_steps(m, B, ts, rc);
            {
                FwdPlan ft;
                const int rct = plan_forward(m, true, B, false, ft);
                check_forward_report(m, 2, B, &ft, nullptr, rct);
            }
            {   // the data-gradient geometries dad_unet_backward hands to its launches: a direct plan_launch of the same op
                size_t nd = 0;
                for (const BwdStep& s : m.bsteps) {
                    if (s.kind != BK_DGRAD) continue;
                    CHECK(nd < ts.dgrads.size(), "B=%d: data-gradient geometries missing", B);
                    if (nd >= ts.dgrads.size()) break;
                    const TrainScratch::Dgrad& d = ts.dgrads[nd++];
                    LaunchGeom g;
                    const int r = plan_launch(m, bwd_op(m, s), B, g);
                    CHECK((r == DAD_OK) == d.ok && std::memcmp(&g.split, &d.g.split, sizeof(SplitPlan)) == 0 && g.cfg == d.g.cfg && g.kc == d.g.kc &&
                          g.ragged == d.g.ragged && g.threads == d.g.threads && g.lds_bytes == d.g.lds_bytes && g.ntiles_n == d.g.ntiles_n &&
                          g.mtiles == d.g.mtiles && g.gx == d.g.gx && g.gy == d.g.gy && g.gz == d.g.gz && g.xcd_gn == d.g.xcd_gn &&
                          g.xcd_mts == d.g.xcd_mts && g.xcd_ntn == d.g.xcd_ntn && g.fused == d.g.fused && g.padded == d.g.padded &&
                          g.windowed == d.g.windowed && g.gn_npt == d.g.gn_npt && g.xswz == d.g.xswz,
                          "%s B=%d: stored data-gradient geometry differs from plan_launch", bwd_op(m, s).name.c_str(), B);
                    if (d.ok) {
                        check_geom(bwd_op(m, s), d.g, B, 0, (size_t)ts.bslab * sizeof(float));
                        CHECK(d.g.gn_npt == 0 && !d.g.fused, "%s B=%d: a data gradient with a GroupNorm pass or a ride", bwd_op(m, s).name.c_str(), B);
                    }
                }
                CHECK(nd == ts.dgrads.size(), "B=%d: %zu data-gradient geometries for %zu steps", B, ts.dgrads.size(), nd);
            }
            std::vector<int32_t> report;                  // dad_debug_backward_plan: what the tests prove their path with
            CHECK(backward_plan_report(m, B, report) == rc, "B=%d: the plan report disagrees about the batch", B);
            CHECK(report.size() == DAD_BP_HEADER + ts.wgrads.size() * DAD_BP_REC_INTS && report[DAD_BP_WGRADS] == (int)ts.wgrads.size(),
                  "B=%d: plan report of %zu ints for %zu weight-gradient launches", B, report.size(), ts.wgrads.size());
            if (report.size() != DAD_BP_HEADER + ts.wgrads.size() * DAD_BP_REC_INTS) continue;
            int multi = 0, most = 0, part_multi = 0;
            CHECK(ts.part == (part_end * B + 63) / 64 * 64, "B=%d: partial sums fill %ld of a %ld-float region", B, part_end * B, ts.part);
            size_t nw = 0;
            for (const BwdStep& s : m.bsteps) {
                if (s.kind != BK_WGRAD) continue;
                CHECK(nw < ts.wgrads.size(), "B=%d: weight-gradient geometries missing", B);
                if (nw >= ts.wgrads.size()) break;
                const WgradShape& sh = ts.wgrads[nw].sh;
                const WgradGeom& g = ts.wgrads[nw++].g;
                const char* key = m.grad_slots[s.slot].key.c_str();
                const long numel = (long)s.M * (s.C0 + s.C1) * s.taps;
                CHECK(g.lds <= dad::kLdsBytes && g.lds == dad::wgrad_lds_floats(g.spc, sh.Lg, sh.Lz, s.taps, s.pad, g.tm, g.tn) * sizeof(float),
                      "%s B=%d: %zu bytes of LDS", key, B, g.lds);
                CHECK(g.spc * sh.Lg <= dad::WG_MAX_GROWS && g.spc * dad::wgrad_segz(sh.Lz, s.taps, s.pad) <= dad::WG_MAX_ZROWS,
                      "%s B=%d: a chunk of %d samples overruns the staging", key, B, g.spc);
                CHECK((g.spc * sh.Lg) % (4 * (8 / (g.tm * g.tn))) == 0, "%s B=%d: chunk rows do not split over the K-groups", key, B);
                CHECK(sh.Lg << sh.wshift == s.Lg && sh.B == B << sh.wshift, "%s B=%d: windows", key, B);
                CHECK(g.sps % g.spc == 0 && (long)g.ksplit * g.sps >= sh.B && (long)(g.ksplit - 1) * g.sps < sh.B,
                      "%s B=%d: batch split %d x %d", key, B, g.ksplit, g.sps);
                CHECK((long)g.gx * 32 * g.tm >= s.M && (long)g.gy * 32 * g.tn >= s.C0 + s.C1, "%s B=%d: grid", key, B);
                CHECK(g.ksplit == 1 || ((long)g.ksplit * numel <= ts.wslab && numel % 4 == 0), "%s B=%d: split slabs", key, B);
                // the kernel's block ks walks samples [ks * sps, min(B, (ks + 1) * sps)) in chunks of spc: the ranges
                // tile [0, B) and none is empty; the chunk counts are what the plan report states
                const int32_t* rec = &report[DAD_BP_HEADER + (nw - 1) * DAD_BP_REC_INTS];
                int at = 0, fullest = 0, last = 0;
                for (int ks = 0; ks < g.ksplit; ++ks) {
                    const int lo = ks * g.sps, hi = std::min(sh.B, (ks + 1) * g.sps);
                    CHECK(lo == at && hi > lo, "%s B=%d: block %d of %d walks samples [%d, %d) after %d", key, B, ks, g.ksplit, lo, hi, at);
                    at = hi;
                    last = (hi - lo + g.spc - 1) / g.spc;
                    fullest = std::max(fullest, last);
                }
                CHECK(at == sh.B, "%s B=%d: the blocks walk %d of %d samples", key, B, at, sh.B);
                CHECK(rec[DAD_BP_REC_CHUNKS] == fullest && rec[DAD_BP_REC_LAST_CHUNKS] == last,
                      "%s B=%d: blocks stage up to %d chunks (the last one %d), the report says %d / %d", key, B, fullest, last,
                      rec[DAD_BP_REC_CHUNKS], rec[DAD_BP_REC_LAST_CHUNKS]);
                CHECK(rec[DAD_BP_REC_TAPS] == s.taps && rec[DAD_BP_REC_TILE] == g.tile && rec[DAD_BP_REC_WINDOWED] == (sh.wshift > 0) &&
                      rec[DAD_BP_REC_SAMPLES] == sh.B && rec[DAD_BP_REC_SPC] == g.spc && rec[DAD_BP_REC_SPS] == g.sps &&
                      rec[DAD_BP_REC_KSPLIT] == g.ksplit, "%s B=%d: plan report record", key, B);
                multi += fullest > 1;
                most = std::max(most, fullest);
                part_multi += sh.B % g.spc != 0 && last > 1;
            }
            CHECK(nw == ts.wgrads.size(), "B=%d: %zu weight-gradient geometries for %zu steps", B, ts.wgrads.size(), nw);
            CHECK(report[DAD_BP_MULTI] == multi && report[DAD_BP_MAX_CHUNKS] == most && report[DAD_BP_PART_MULTI] == part_multi,
                  "B=%d: plan report counts %d multi-chunk launches (most %d chunks, %d part filled), the geometries give %d (%d, %d)", B,
                  report[DAD_BP_MULTI], report[DAD_BP_MAX_CHUNKS], report[DAD_BP_PART_MULTI], multi, most, part_multi);
        }
    }
    (void)bwd_launches;
    printf("  %-14s prec=%d: %zu launches in the plan, %zu buffers, %ld floats/sample, %ld launch geometries checked\n",
           a.name, precision, P.convs.size(), P.bufs.size(), P.floats_per_sample, launches);
    (void)cc_plans;
}

int main(int argc, char** argv) {
    const bool quick = argc > 1 && std::string(argv[1]) == "--quick";
    std::vector<Arch> archs = {
        {"tiny", 6, 32, 32, 32, {1, 2, 4}, true},
        {"tiny4", 8, 32, 32, 32, {1, 2, 2, 4}, true},
        {"tiny_td64", 6, 32, 64, 32, {1, 2, 4}, true},
        {"pointmaze", 6, 128, 128, 32, {1, 2, 4}, true},
        {"halfcheetah", 23, 256, 256, 32, {1, 4, 8}, !quick},
        {"door", 67, 256, 256, 32, {1, 2, 4, 8}, !quick},
        {"shrink", 6, 32, 32, 32, {1, 4, 2}, true},
        {"shrink2", 5, 32, 32, 32, {1, 4, 2, 1}, true},
        {"single", 3, 32, 32, 32, {1}, true},
        {"h8", 8, 128, 128, 8, {1, 4}, true},
        {"h64", 23, 64, 64, 64, {1, 1, 2}, true},
        {"h128", 6, 128, 128, 128, {1, 2, 4}, true},
        {"h128w", 23, 256, 256, 128, {1, 4, 8}, false},
        {"pointmaze_k3", 6, 128, 128, 32, {1, 2, 4}, true, 3},
        {"tiny_k7", 8, 64, 64, 32, {1, 2}, true, 7},
        {"wide_k3", 23, 256, 256, 32, {1, 4, 8}, !quick, 3},
        {"wide_k7", 9, 256, 256, 16, {1, 8}, false, 7},
        {"h128_k7", 6, 128, 128, 128, {1, 2}, true, 7},
        {"shrink_k7", 5, 32, 32, 32, {1, 4, 2}, true, 7},
        {"d48_padded", 6, 64, 48, 32, {1, 2}, true, 5, {48, 96}},          // --dim 48 as the engine runs it
        {"d40_padded", 5, 64, 40, 32, {1, 2, 2}, true, 5, {40, 80, 120}},   // 40 / 80 / 120 -> 64 / 128 / 128
        {"h24_padded", 6, 32, 32, 32, {1, 2, 4}, true, 5, {}, 24},          // horizon 24 as the engine runs it (32)
        {"h100_padded", 11, 64, 64, 128, {1, 2, 4}, true, 5, {}, 100},      // 100 / 50 / 25 positions in 128 / 64 / 32
        {"h48_d48", 6, 64, 48, 64, {1, 2}, true, 3, {48, 96}, 48},          // both paddings + kernel_size 3
    };
    // the fuzz generator's space (tests/fuzz_parity.py), deterministic sweep
    std::mt19937 rng(7);
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    std::vector<std::string> names;
    names.reserve(64);
    for (int it = 0; it < 40; ++it) {
        const int dim = pick({32, 64, 128, 256});
        const int nlev = pick({1, 2, 3, 4});
        std::vector<int> mults{1};
        int mx = 1;
        for (int i = 1; i < nlev; ++i) { mults.push_back(pick({1, 2, 4, 8})); mx = std::max(mx, mults.back()); }
        const int H = pick({8, 16, 32, 64});
        const int td = 2 + (int)(rng() % 23);
        if (mx * dim > 2048) continue;
        names.push_back("fuzz" + std::to_string(it));
        archs.push_back({names.back().c_str(), td, dim, dim, H, mults, mx * dim <= 512, it % 4 == 3 ? pick({3, 7}) : 5});
    }
    for (const Arch& a : archs)
        for (int prec : {DAD_PREC_FP32, DAD_PREC_F16X3}) check_arch(a, prec);

    // refusals are messages
    dad_cfg bad{};
    bad.transition_dim = 6; bad.dim = 48; bad.time_dim = 48; bad.n_levels = 2;
    bad.channels[0] = 48; bad.channels[1] = 96; bad.kernel_size = 5; bad.horizon = 32; bad.n_timesteps = 10;
    CHECK(check_cfg(&bad) == DAD_E_INVALID && g_err[0] != 0, "48 channels accepted");
    bad.dim = 32; bad.channels[0] = 32; bad.channels[1] = 64; bad.horizon = 4;
    CHECK(check_cfg(&bad) == DAD_E_INVALID, "horizon 4 with two levels accepted");
    CHECK(check_cfg(nullptr) == DAD_E_INVALID, "null cfg accepted");

    // split-f16 images: round trip hi + lo * 2^-11 reproduces the scaled weight to 2^-22
    {
        std::vector<float> w(64);
        uint64_t st = 99;
        for (float& v : w) v = synth(st) * 0.3f;
        w[5] = 0.0f; w[6] = 1e-8f;
        std::vector<float> img = w;
        const int s = split_f16_image(img);
        for (size_t g = 0; g < w.size(); g += 16)
            for (int j = 0; j < 16; ++j) {
                uint16_t hb, lb;
                std::memcpy(&hb, (const char*)&img[g] + 2 * j, 2);
                std::memcpy(&lb, (const char*)&img[g + 8] + 2 * j, 2);
                _Float16 h, l;
                std::memcpy(&h, &hb, 2); std::memcpy(&l, &lb, 2);
                const double back = ((double)(float)h + (double)(float)l / 2048.0) * std::ldexp(1.0, -s);
                CHECK(std::fabs(back - w[g + j]) <= std::ldexp(std::fabs((double)w[g + j]), -21) + 1e-12,
                      "split image element %zu: %g vs %g", g + j, back, (double)w[g + j]);
            }
    }
    // sinusoid table: shape and a few exact entries
    {
        const std::vector<float> e = sinusoid_table(10, 32);
        CHECK(e.size() == 320 && e[0] == 0.0f && e[16] == 1.0f, "sinusoid table t=0");
        CHECK(std::fabs(e[32] - std::sin(1.0f)) < 1e-7, "sinusoid table t=1");
    }
    // projection plan: every (D, batch), with and without scratch, for dad_project and the violation, either fits
    // LDS on a grid that covers the batch (and, as a GEMM, the columns of P) or is refused; the GEMM form needs
    // scratch for the whole batch and 32 trajectories, and never serves the violation
    {
        long plans = 0, refused = 0, forms[3] = {0, 0, 0};
        for (int D : {1, 7, 33, 63, 64, 65, 196, 511, 512, 524, 602, 603, 753, 2183, 2409, 2410, 4096, 100000})
            for (int batch : {1, 3, 4, 31, 32, 33, 256, 512, 513, 515, 4096})
                for (int with_scratch : {0, 1, 2})
                    for (int violation : {0, 1}) {
                        const size_t x_bytes = (size_t)batch * 96 * sizeof(float);
                        const size_t scratch = with_scratch == 0 ? 0 : with_scratch == 1 ? x_bytes - 4 : x_bytes;
                        const ProjectPlan q = plan_project(D, batch, x_bytes, scratch, violation != 0);
                        ++plans; refused += q.refused;
                        CHECK(q.form >= DAD_PP_ROW1 && q.form <= DAD_PP_GEMM, "D=%d B=%d: form %d", D, batch, q.form);
                        ++forms[q.form];
                        CHECK(q.refused || q.lds_bytes <= dad::kLdsBytes, "D=%d B=%d: %zu bytes of LDS accepted", D, batch, q.lds_bytes);
                        CHECK((long)q.gx * q.rows_per_block >= batch && (long)(q.gx - 1) * q.rows_per_block < batch,
                              "D=%d B=%d: grid x %u of %d rows", D, batch, q.gx, q.rows_per_block);
                        if (q.form == DAD_PP_GEMM) {
                            CHECK(!q.refused && !violation && batch >= 32 && scratch >= x_bytes, "D=%d B=%d: GEMM form", D, batch);
                            CHECK(q.rows_per_block == 32 && (long)q.gy * 32 >= D && (long)(q.gy - 1) * 32 < D, "D=%d: grid y %u", D, q.gy);
                            CHECK(q.lds_bytes >= (size_t)4 * 32 * dad::PG_AS * sizeof(float), "GEMM exchange tile");
                        } else {
                            CHECK(q.gy == 1 && q.rows_per_block == (q.form == DAD_PP_ROW4 ? 4 : 1), "D=%d B=%d: rows", D, batch);
                            CHECK(q.lds_bytes == (size_t)q.rows_per_block * (1 + dad::PROJ_KP) * D * sizeof(float), "D=%d: row LDS", D);
                            CHECK(q.form == DAD_PP_ROW1 || batch > 512, "D=%d B=%d: four rows per block within one wave of blocks", D, batch);
                        }
                        CHECK(q.refused == (q.form != DAD_PP_GEMM && (size_t)(1 + dad::PROJ_KP) * D * sizeof(float) > dad::kLdsBytes),
                              "D=%d B=%d: refusal", D, batch);
                    }
        CHECK(forms[0] && forms[1] && forms[2] && refused, "the projection sweep misses a form or the refusal");
        printf("  projection plan: %ld plans (%ld row1, %ld row4, %ld gemm), %ld refused\n", plans, forms[0], forms[1], forms[2], refused);
    }
    CHECK(g_reports > 0, "no forward-plan report was compared");
    CHECK(g_step_reports > 0, "no backward-step report was compared");
    CHECK(g_halo8_reports > 0 && g_halo8_records > 0, "no conv_halo8_f32 launch report was compared (%ld reports, %ld records)", g_halo8_reports, g_halo8_records);
    printf("  halo8 plan: %ld reports, %ld launch records\n", g_halo8_reports, g_halo8_records);
    if (g_failures) { fprintf(stderr, "%d host-logic checks FAILED\n", g_failures); return 1; }
    printf("host logic ok (%ld forward-plan and %ld backward-step reports equal the descriptions they were read from)\n", g_reports,
           g_step_reports);
    return 0;
}
