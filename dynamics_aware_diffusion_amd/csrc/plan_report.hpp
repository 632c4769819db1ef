// plan_report.hpp — the plans of host_plan.hpp written down as the flat int32 reports of include/dad.h (dad_debug_*_plan,
// dad_debug_backward_steps).  Nothing here decides anything: an *_encode function writes down a description the entry
// points replay, an *_report function plans the call as its entry point does and encodes that.  The layouts are the
// *_LIST lists of include/dad.h: every field is written by its constant (the order of the statements carries no
// meaning), and report_layout() hands the same lists to the binding as text.  Plain C++17, no HIP.
#pragma once
#include "host_plan.hpp"

namespace dadhost {

// ------------------------------------------------------------------ the layouts as text (dad_debug_report_layout)
// One row per report: its header first, then its records and the values its fields take.  S: one list of
// include/dad.h, named by its length constant; K: a kind of backward step, whose record starts with DAD_BS_KIND.
#define DAD_LAYOUT_TEXT(NAME, name, span, doc) " " #NAME " " #name " " #span
#define S(LENGTH) #LENGTH LENGTH##_LIST(DAD_LAYOUT_TEXT)
#define K(LENGTH) #LENGTH DAD_BS_KIND_FIELD(DAD_LAYOUT_TEXT) LENGTH##_LIST(DAD_LAYOUT_TEXT)
constexpr int kMaxReportSections = 9;
constexpr const char* kReportLayouts[][kMaxReportSections] = {
    {S(DAD_FP_HEADER), S(DAD_FP_REC_INTS), S(DAD_FP_CC_INTS), S(DAD_FP_FINALS), S(DAD_FP_FAMILIES)},
    {S(DAD_H8_HEADER), S(DAD_H8_INTS)},
    {S(DAD_SEAM_INTS), S(DAD_SEAM_BUFS)},
    {S(DAD_PP_INTS), S(DAD_PP_FORMS)},
    {S(DAD_BP_HEADER), S(DAD_BP_REC_INTS)},
    {S(DAD_BS_HEADER), S(DAD_BS_REC_INTS), S(DAD_BS_KINDS), K(DAD_BS_BIAS_INTS), K(DAD_BS_WGRAD_INTS), K(DAD_BS_DGRAD_INTS),
     K(DAD_BS_GN_INTS), K(DAD_BS_RESID_INTS), K(DAD_BS_COLS_INTS)},
    {S(DAD_OP_HEADER), S(DAD_OP_REC_INTS), S(DAD_OP_TG_MODES)},
    {S(DAD_OS_HEADER), S(DAD_OS_REC_INTS)},
    {S(DAD_KL_HEADER), S(DAD_FAMILIES)},
    {S(DAD_VG_INTS), S(DAD_VG_FORMS)},
    {S(DAD_GD_INTS), S(DAD_GD_ACTS), S(DAD_GD_REFUSALS)},
    {S(DAD_DO_HEADER), S(DAD_DO_REC_INTS), S(DAD_DO_KINDS)},
};
#undef K
#undef S
#undef DAD_LAYOUT_TEXT
static_assert(DAD_BS_BIAS_INTS == DAD_BS_REC_INTS && DAD_BS_WGRAD_INTS == DAD_BS_REC_INTS && DAD_BS_DGRAD_INTS == DAD_BS_REC_INTS &&
              DAD_BS_GN_INTS == DAD_BS_REC_INTS && DAD_BS_RESID_INTS == DAD_BS_REC_INTS && DAD_BS_COLS_INTS == DAD_BS_REC_INTS,
              "every kind of backward step fills a whole record: a DAD_BS_*_UNUSED span is off");
inline const char* report_layout(int report, int section) {
    if (report < 0 || report >= (int)std::size(kReportLayouts) || section < 0 || section >= kMaxReportSections) return nullptr;
    return kReportLayouts[report][section];
}

// a new record of `ints` zeros at the end of `r` (valid until `r` grows again)
inline int32_t* new_record(std::vector<int32_t>& r, int ints) {
    r.resize(r.size() + (size_t)ints, 0);
    return r.data() + r.size() - ints;
}

// dad_debug_backward_plan: which kernels one training step takes at batch B, read from what dad_unet_forward_train and
// dad_unet_backward replay: plan_forward of the training plan, train_scratch.
inline int backward_plan_report(const HostModel& m, int B, std::vector<int32_t>& r) {
    TrainScratch ts;
    FwdPlan fwd;
    plan_forward(m, true, B, false, fwd);
    const int rc = train_scratch(m, B, ts);
    r.assign(DAD_BP_HEADER, 0);
    r[DAD_BP_RECORD_INTS] = DAD_BP_REC_INTS;
    size_t nw = 0;
    auto conv = [&](const LaunchGeom& g, int at) { if (g.cfg >= 0) ++r[at + 2 * g.cfg + (g.split.kslices > 1 ? 1 : 0)]; };
    for (const FwdLaunch& l : fwd.launches) conv(l.g, DAD_BP_FWD);
    for (const TrainScratch::Dgrad& d : ts.dgrads) conv(d.g, DAD_BP_DGRAD);
    for (const BwdStep& s : m.bsteps) {
        if (s.kind != BK_WGRAD) continue;
        const WgradShape& sh = ts.wgrads[nw].sh;
        const WgradGeom& g = ts.wgrads[nw++].g;
        const int fullest = (std::min(g.sps, sh.B) + g.spc - 1) / g.spc;
        const int last = (sh.B - (g.ksplit - 1) * g.sps + g.spc - 1) / g.spc;
        const bool part = sh.B % g.spc != 0;
        const int ti = (int)(std::find(std::begin(kWgradTaps), std::end(kWgradTaps), s.taps) - std::begin(kWgradTaps));
        ++r[DAD_BP_WGRADS];
        r[DAD_BP_MULTI] += fullest > 1;
        r[DAD_BP_MAX_CHUNKS] = std::max(r[DAD_BP_MAX_CHUNKS], fullest);
        r[DAD_BP_MAX_KSPLIT] = std::max(r[DAD_BP_MAX_KSPLIT], g.ksplit);
        r[DAD_BP_PART] += part;
        r[DAD_BP_PART_MULTI] += part && last > 1;
        r[DAD_BP_WINDOWED] += sh.wshift > 0;
        ++r[DAD_BP_TILE + g.tile];
        if (ti < (int)std::size(kWgradTaps)) ++r[DAD_BP_TAPS_TILE + 4 * ti + g.tile];
        int32_t* rec = new_record(r, DAD_BP_REC_INTS);
        rec[DAD_BP_REC_TAPS] = s.taps; rec[DAD_BP_REC_TILE] = g.tile; rec[DAD_BP_REC_WINDOWED] = sh.wshift > 0;
        rec[DAD_BP_REC_SAMPLES] = sh.B; rec[DAD_BP_REC_SPC] = g.spc; rec[DAD_BP_REC_SPS] = g.sps;
        rec[DAD_BP_REC_KSPLIT] = g.ksplit; rec[DAD_BP_REC_CHUNKS] = fullest; rec[DAD_BP_REC_LAST_CHUNKS] = last;
    }
    return rc;
}

// dad_debug_backward_steps: everything dad_unet_backward replays at batch B, step by step.  backward_steps_encode writes
// down m.bsteps / m.bsums with the geometry `ts` (train_scratch) the entry point launches from.
inline void backward_steps_encode(const HostModel& m, int B, const TrainScratch& ts, std::vector<int32_t>& r) {
    const int H = m.cfg.horizon, Hr = traj_horizon(m);
    r.assign(DAD_BS_HEADER, 0);
    r[DAD_BS_RECORD_INTS] = DAD_BS_REC_INTS;
    r[DAD_BS_BATCH] = B;
    r[DAD_BS_COLSUMS_LAUNCHES] = col_sums_launches(m);
    r[DAD_BS_COLSUMS_ENTRIES] = (int32_t)m.bsums.size();
    for (const BwdSum& q : m.bsums) r[DAD_BS_COLSUMS_WIDEST] = std::max(r[DAD_BS_COLSUMS_WIDEST], (int32_t)q.C);
    r[DAD_BS_PADCOPY] = Hr != H;
    r[DAD_BS_HORIZON] = H;
    r[DAD_BS_REAL_HORIZON] = Hr;
    r[DAD_BS_DX] = m.bdx;
    size_t nw = 0;
    for (const BwdStep& s : m.bsteps) {
        int32_t* rec = new_record(r, DAD_BS_REC_INTS);
        ++r[DAD_BS_STEPS];
        rec[DAD_BS_KIND] = (int32_t)s.kind;
        switch (s.kind) {
            case BK_BIAS:
                rec[DAD_BS_BIAS_ROWS] = s.rows; rec[DAD_BS_BIAS_C] = s.C;
                break;
            case BK_WGRAD: {
                if (nw >= ts.wgrads.size()) break;
                const WgradShape& sh = ts.wgrads[nw].sh;
                const WgradGeom& g = ts.wgrads[nw++].g;
                const int Ctot = s.C0 + s.C1, wm = 32 * g.tm, wn = 32 * g.tn;
                const long numel = (long)s.M * Ctot * s.taps;
                rec[DAD_BS_WG_TAPS] = s.taps; rec[DAD_BS_WG_TILE] = g.tile; rec[DAD_BS_WG_WINDOWED] = sh.wshift > 0;
                rec[DAD_BS_WG_M] = s.M; rec[DAD_BS_WG_C0] = s.C0; rec[DAD_BS_WG_C1] = s.C1;
                rec[DAD_BS_WG_STRIDE] = s.stride; rec[DAD_BS_WG_PAD] = s.pad; rec[DAD_BS_WG_LG] = sh.Lg; rec[DAD_BS_WG_LZ] = sh.Lz;
                rec[DAD_BS_WG_GX] = (int32_t)g.gx; rec[DAD_BS_WG_GY] = (int32_t)g.gy;
                rec[DAD_BS_WG_RAGGED] = g.tile == 3;
                rec[DAD_BS_WG_CONCAT_INSIDE] = s.C1 > 0 && s.C0 % wn != 0;
                rec[DAD_BS_WG_EDGE_M] = s.M % wm != 0;
                rec[DAD_BS_WG_EDGE_C] = Ctot % wn != 0;
                rec[DAD_BS_WG_SWAPPED] = s.in.sp == BSP_ACT || s.in.sp == BSP_X;
                rec[DAD_BS_WG_KSPLIT] = g.ksplit;
                rec[DAD_BS_WG_SLAB_N4] = g.ksplit > 1 ? (int32_t)(numel / 4) : 0;
                rec[DAD_BS_WG_SAMPLES] = sh.B; rec[DAD_BS_WG_SPC] = g.spc; rec[DAD_BS_WG_SPS] = g.sps;
                rec[DAD_BS_WG_CHUNKS] = (std::min(g.sps, sh.B) + g.spc - 1) / g.spc;
                rec[DAD_BS_WG_LAST_CHUNKS] = (sh.B - (g.ksplit - 1) * g.sps + g.spc - 1) / g.spc;
                break;
            }
            case BK_DGRAD:
                rec[DAD_BS_DG_CONV] = s.conv; rec[DAD_BS_DG_SUB] = s.sub; rec[DAD_BS_DG_WRITE] = (int32_t)s.write;
                break;
            case BK_GN: {
                const GnBwdShape q = gn_bwd_shape(m.tplan.convs[s.conv]);
                rec[DAD_BS_GN_NV] = s.nv; rec[DAD_BS_GN_CPG] = q.cpg; rec[DAD_BS_GN_L] = q.L; rec[DAD_BS_GN_LREAL] = q.lreal;
                rec[DAD_BS_GN_CPG_REAL] = q.cpg_real; rec[DAD_BS_GN_DTEMB] = q.dtemb; rec[DAD_BS_GN_C] = q.C;
                rec[DAD_BS_GN_SHORT_PAIR] = q.cpg / 4 * q.L < 64;
                break;
            }
            case BK_RESID:
                rec[DAD_BS_RS_WRITE] = (int32_t)s.write; rec[DAD_BS_RS_N] = (int32_t)std::min<long>(s.n, INT32_MAX);
                rec[DAD_BS_RS_TO_X] = s.out.sp == BSP_DX;
                break;
            case BK_COLS:
                rec[DAD_BS_CL_C] = s.C; rec[DAD_BS_CL_OFF] = s.off; rec[DAD_BS_CL_LD] = s.ld; rec[DAD_BS_CL_ROWS] = s.rows;
                rec[DAD_BS_CL_WRITE] = (int32_t)s.write;
                break;
        }
    }
}
inline int backward_steps_report(const HostModel& m, int B, std::vector<int32_t>& r) {
    TrainScratch ts;
    const int rc = train_scratch(m, B, ts);
    backward_steps_encode(m, B, ts, r);
    return rc;
}

// dad_debug_objective_plan: the time chain of one fused objective step at batch B, read from the list
// dad_train_objective_forward / _backward replay (ObjectivePlan::time).
inline int objective_plan_report(const HostModel& m, int B, std::vector<int32_t>& r) {
    ObjectivePlan p;
    const int rc = objective_plan(m, B, true, p);
    const long n = (long)B * traj_horizon(m) * m.cfg.transition_dim;
    r.assign(DAD_OP_HEADER, 0);
    r[DAD_OP_LOSS_BLOCKS] = p.o.loss_blocks;
    r[DAD_OP_KSLICES] = p.o.kslices;
    r[DAD_OP_KSLICE] = p.o.kslice;
    r[DAD_OP_TEMB_WIDTH] = m.tplan.temb_width;
    r[DAD_OP_BLOCKS] = (int32_t)time_block_list(m).size();
    r[DAD_OP_N] = (int32_t)std::min<long>(n, INT32_MAX);
    r[DAD_OP_RECORD_INTS] = DAD_OP_REC_INTS;
    r[DAD_OP_LAUNCHES] = (int32_t)p.time.size();
    for (const TimeLaunch& l : p.time) {
        const bool gemm = l.mode != DAD_OP_TG_DTEMB;
        const int full = std::min(l.kslice, l.K), last = l.K - (l.kslices - 1) * l.kslice;
        int32_t* rec = new_record(r, DAD_OP_REC_INTS);
        rec[DAD_OP_REC_MODE] = l.mode; rec[DAD_OP_REC_M] = l.M; rec[DAD_OP_REC_N] = l.N; rec[DAD_OP_REC_K] = l.K;
        rec[DAD_OP_REC_GRID_X] = (int32_t)l.gx(); rec[DAD_OP_REC_GRID_Y] = (int32_t)l.gy(); rec[DAD_OP_REC_GRID_Z] = (int32_t)l.gz();
        rec[DAD_OP_REC_CHUNKS] = gemm ? (full + 31) / 32 : 0; rec[DAD_OP_REC_LAST_CHUNKS] = gemm ? (last + 31) / 32 : 0;
        rec[DAD_OP_REC_KTAIL] = gemm ? l.K % 32 : 0; rec[DAD_OP_REC_KSLICE] = l.kslice;
    }
    return rc;
}

// dad_debug_dynamics_objective_plan: what dad_train_dynamics_objective_forward / _backward lay out and launch beyond
// the fused objective, read from the plan they replay (dynamics_objective_plan).
inline int dynamics_objective_plan_report(const HostModel& m, int B, int state_dim, int observation_dim, int action_dim, int form,
                                          std::vector<int32_t>& r) {
    DynamicsObjectivePlan p;
    const int rc = dynamics_objective_plan(m, B, state_dim, observation_dim, action_dim, form, true, p);
    if (p.launches.empty()) return rc;             // (the shape itself was refused: nothing was planned)
    const auto i32 = [](size_t v) { return (int32_t)std::min<size_t>(v, INT32_MAX); };
    r.assign(DAD_DO_HEADER, 0);
    r[DAD_DO_FORM] = p.vg.form; r[DAD_DO_D] = p.D; r[DAD_DO_HORIZON] = p.horizon; r[DAD_DO_COL_BLOCKS] = p.vg.col_blocks;
    r[DAD_DO_REFUSED] = p.vg.refused;
    r[DAD_DO_SAVED_BASE] = i32(p.saved_base); r[DAD_DO_SAVED_BYTES] = i32(p.saved_bytes);
    r[DAD_DO_SCRATCH_BASE] = i32(p.scratch_base); r[DAD_DO_SCRATCH_BYTES] = i32(p.scratch_bytes);
    r[DAD_DO_R_OFFSET] = i32((size_t)p.r); r[DAD_DO_PART_OFFSET] = i32((size_t)p.part);
    r[DAD_DO_VIOLATION_OFFSET] = i32((size_t)p.violation); r[DAD_DO_G_OFFSET] = i32((size_t)p.g);
    r[DAD_DO_OBJECTIVE_LAUNCHES] = (int32_t)p.obj.time.size();
    r[DAD_DO_FWD_LAUNCHES] = p.fwd_launches;
    r[DAD_DO_RECORD_INTS] = DAD_DO_REC_INTS;
    r[DAD_DO_LAUNCHES] = (int32_t)p.launches.size();
    for (const DynLaunch& l : p.launches) {
        int32_t* rec = new_record(r, DAD_DO_REC_INTS);
        rec[DAD_DO_REC_KIND] = l.kind; rec[DAD_DO_REC_GRID_X] = (int32_t)l.gx; rec[DAD_DO_REC_GRID_Y] = (int32_t)l.gy;
        rec[DAD_DO_REC_THREADS] = l.threads; rec[DAD_DO_REC_LDS_BYTES] = i32(l.lds_bytes); rec[DAD_DO_REC_ROWS_PER_BLOCK] = l.rows_per_block;
    }
    return rc;
}

// dad_debug_forward_plan: what one forward evaluation (modes 0 .. 2) or the data-gradient half of one backward pass
// (mode 3) launches at a batch.  `f`: plan_forward's description (modes 0 .. 2), `ts`: train_scratch's (mode 3).
inline void forward_plan_encode(const HostModel& m, int mode, int batch, const FwdPlan* f, const TrainScratch* ts,
                                std::vector<int32_t>& r) {
    r.assign(DAD_FP_HEADER, 0);
    r[DAD_FP_MODE] = mode;
    r[DAD_FP_BATCH] = batch;
    r[DAD_FP_FINAL_KERNEL] = DAD_FP_FINAL_NONE;
    auto conv = [&](int index, int sub, const ConvOp& op, const LaunchGeom& g) {
        const int bn = g.cfg >= 0 ? kTiles[g.cfg].BN : 0;
        int32_t* rec = new_record(r, DAD_FP_REC_INTS);
        ++r[DAD_FP_RECORDS];
        rec[DAD_FP_REC_CONV] = index; rec[DAD_FP_REC_SUB] = sub; rec[DAD_FP_REC_CFG] = g.cfg;
        rec[DAD_FP_REC_TAPS] = op.taps; rec[DAD_FP_REC_STRIDE] = op.stride; rec[DAD_FP_REC_FLAGS] = launch_flags(op, g);
        rec[DAD_FP_REC_KC] = g.kc; rec[DAD_FP_REC_KSLICES] = g.split.kslices; rec[DAD_FP_REC_GN_NPT] = g.gn_npt;
        rec[DAD_FP_REC_NTILES_N] = g.ntiles_n; rec[DAD_FP_REC_MTILES] = g.mtiles;
        rec[DAD_FP_REC_PART_TILE] = g.cfg >= 0 && op.Lout <= bn && batch % (bn / op.Lout) != 0;
        rec[DAD_FP_REC_FAMILY] = !g.halo8 ? DAD_FP_FAMILY_GEMM : g.halo8w ? DAD_FP_FAMILY_HALO8W : DAD_FP_FAMILY_HALO8;
    };
    r[DAD_FP_RECORD_INTS] = DAD_FP_REC_INTS;
    if (mode == 3) {
        size_t nd = 0;
        for (const BwdStep& s : m.bsteps)
            if (s.kind == BK_DGRAD && nd < ts->dgrads.size()) conv(s.conv, s.sub, bwd_op(m, s), ts->dgrads[nd++].g);
        return;
    }
    const Plan& plan = f->train ? m.tplan : m.plan;
    r[DAD_FP_FINAL_GX] = (int32_t)f->final_gx;
    r[DAD_FP_FINAL_GY] = (int32_t)f->final_gy;
    r[DAD_FP_FINAL_KERNEL] = f->cc.ok ? DAD_FP_FINAL_CC : DAD_FP_FINAL_POSTERIOR;
    if (!f->cc.ok) {
        for (const FwdLaunch& l : f->launches) conv(l.conv, 0, plan.convs[l.conv], l.g);
        return;
    }
    r[DAD_FP_SMALL] = 1;
    r[DAD_FP_RECORD_INTS] = DAD_FP_CC_INTS;
    for (size_t i = 0; i < f->cc.ops.size(); ++i) {
        const CcOp& o = f->cc.ops[i];
        if (!o.launched) continue;
        const ConvOp& op = plan.convs[i];
        int32_t* rec = new_record(r, DAD_FP_CC_INTS);
        ++r[DAD_FP_RECORDS];
        rec[DAD_FP_CC_CONV] = (int32_t)i; rec[DAD_FP_CC_TAPS] = op.taps; rec[DAD_FP_CC_STRIDE] = op.stride;
        rec[DAD_FP_CC_WIDE] = o.wide; rec[DAD_FP_CC_RIDE] = op.ride; rec[DAD_FP_CC_BIG] = o.big; rec[DAD_FP_CC_RIDE_IN] = o.ride_in;
        rec[DAD_FP_CC_TILE_ROWS] = o.tile_rows; rec[DAD_FP_CC_WINDOWED] = op.Lout > 32;
        rec[DAD_FP_CC_SLICE_CH] = o.slice_ch; rec[DAD_FP_CC_KSLICES] = o.kslices; rec[DAD_FP_CC_NTILES] = o.ntiles;
        rec[DAD_FP_CC_RES_KIND] = o.res_kind;
    }
}
inline int forward_plan_report(const HostModel& m, int batch, int mode, std::vector<int32_t>& r) {
    FwdPlan f;
    TrainScratch ts;
    const int rc = mode == 3 ? train_scratch(m, batch, ts) : plan_forward(m, mode == 2, batch, mode == 0, f);
    forward_plan_encode(m, mode, batch, &f, &ts, r);
    return rc;
}
// dad_debug_halo8_plan: the conv_halo8_f32 launches of `f` (plan_forward on m.plan, modes 0 / 1) with what the kernel
// makes of the ConvParams that conv_params / conv_io of dad_lib.hip fill from the same ConvOp and LaunchGeom.
// `rows`: the evaluation indexes its time embedding per sample (dad_unet_forward_rows).
inline void halo8_plan_encode(const HostModel& m, const FwdPlan& f, bool rows, std::vector<int32_t>& r) {
    r.assign(DAD_H8_HEADER, 0);
    r[DAD_H8_RECORD_INTS] = DAD_H8_INTS;
    if (f.train || f.cc.ok) return;
    for (const FwdLaunch& l : f.launches) {
        if (!l.g.halo8) continue;
        const ConvOp& op = m.plan.convs[l.conv];
        const LaunchGeom& g = l.g;
        const TileCfg& t = kTiles[g.cfg];
        const bool gn = !op.norm.empty() && g.gn_npt == 0;
        const bool temb = op.temb_off >= 0;
        // waves per pair: the kernel's own `wpp` is lpp >> 6, 0 for a pair inside one wave; the report says 1 there
        const int lpp = gn ? dad::halo8_lanes_per_pair(t.BM, g.threads, op.cout / 8) : 0;
        int32_t* rec = new_record(r, DAD_H8_INTS);
        ++r[DAD_H8_RECORDS];
        rec[DAD_H8_CONV] = l.conv; rec[DAD_H8_CFG] = g.cfg; rec[DAD_H8_RIDE] = g.fused;
        rec[DAD_H8_CHUNKS] = (op.cin0 + op.cin1) / 32; rec[DAD_H8_SRC1_CHUNK] = op.src1 >= 0 ? op.cin0 / 32 : -1;
        rec[DAD_H8_RES] = op.res == -2 || op.res >= 0; rec[DAD_H8_TEMB] = temb; rec[DAD_H8_PER_ROW] = rows && temb;
        rec[DAD_H8_GN] = gn; rec[DAD_H8_WPP] = gn ? std::max(1, lpp >> 6) : 0;
        rec[DAD_H8_XCD_GN] = g.xcd_gn; rec[DAD_H8_MTILES] = g.mtiles; rec[DAD_H8_NTILES_N] = g.ntiles_n;
        rec[DAD_H8_PART_TILE] = f.batch % (t.BN / op.Lout) != 0;
    }
}

// dad_debug_seam_plan: what plan_seam says of the loop's description at a batch; out[DAD_SEAM_INTS].
inline int seam_plan_report(const HostModel& m, int batch, bool projection, int32_t* out) {
    FwdPlan f;
    const int rc = plan_forward(m, false, batch, true, f);      // (a batch the loop refuses is refused here too)
    if (rc != DAD_OK) return rc;
    const SeamPlan s = plan_seam(m, f, projection);
    const bool on = s.taken();
    out[DAD_SEAM_TAKEN] = on;
    out[DAD_SEAM_REASON] = s.why;
    out[DAD_SEAM_GRID] = on ? (int32_t)s.grid : 0;
    out[DAD_SEAM_THREADS] = on ? s.threads : 0;
    out[DAD_SEAM_LDS_BYTES] = on ? (int32_t)s.lds_bytes : 0;
    out[DAD_SEAM_TILE] = on ? s.cfg : -1;
    out[DAD_SEAM_UNITS] = on ? s.units : 0;
    out[DAD_SEAM_SPT] = on ? s.spt : 0;
    out[DAD_SEAM_LAST] = on ? s.last : 0;
    out[DAD_SEAM_BUFFERS] = on ? s.buffers : -1;
    out[DAD_SEAM_DIM] = on ? s.dim : 0;
    out[DAD_SEAM_TILE0] = on ? (int32_t)s.tile0 : -1;
    return DAD_OK;
}

// dad_debug_project_plan: plan_project for trajectories of this shape; out[DAD_PP_INTS].
inline int project_plan_report(int state_dim, int observation_dim, int action_dim, int batch, int horizon, size_t scratch_bytes,
                               bool violation, int32_t* out) {
    const long D = (long)(horizon + 1) * state_dim + (long)horizon * action_dim;
    if (D > INT32_MAX / 64) return fail(DAD_E_INVALID, "projection dimension D=%ld too large", D);
    const size_t x_bytes = (size_t)batch * horizon * (observation_dim + action_dim) * sizeof(float);
    const ProjectPlan q = plan_project((int)D, batch, x_bytes, scratch_bytes, violation);
    out[DAD_PP_FORM] = q.form;
    out[DAD_PP_ROWS_PER_BLOCK] = q.rows_per_block;
    out[DAD_PP_GX] = (int32_t)q.gx;
    out[DAD_PP_GY] = (int32_t)q.gy;
    out[DAD_PP_LDS_BYTES] = (int32_t)std::min<size_t>(q.lds_bytes, INT32_MAX);
    out[DAD_PP_REFUSED] = q.refused;
    return DAD_OK;
}

// The plan of one dad_projection_violation_fwd / _bwd pair, after the checks on the shape that every entry point of the
// pair makes (and dad_debug_violation_grad_plan with them).  A forced row form that does not fit is planned, not refused.
inline int violation_grad_plan_checked(int state_dim, int observation_dim, int action_dim, int batch, int horizon, int form,
                                       int& D_out, ViolationGradPlan& q) {
    if (batch <= 0 || horizon <= 0) return fail(DAD_E_INVALID, "violation gradient: batch=%d, horizon=%d must be positive", batch, horizon);
    if (state_dim <= 0 || action_dim <= 0 || state_dim > observation_dim)
        return fail(DAD_E_INVALID, "violation gradient: state_dim=%d must lie in 1 .. observation_dim=%d, action_dim=%d be positive",
                    state_dim, observation_dim, action_dim);
    if (form < -1 || form > 1) return fail(DAD_E_INVALID, "violation gradient: form=%d is none of -1 (planned), 0 (row), 1 (gemm)", form);
    const long D = (long)(horizon + 1) * state_dim + (long)horizon * action_dim;
    if (D > INT32_MAX / 64) return fail(DAD_E_INVALID, "projection dimension D=%ld too large", D);
    D_out = (int)D;
    q = plan_violation_grad((int)D, batch, (long)horizon * (observation_dim + action_dim), form);
    return DAD_OK;
}
// dad_debug_violation_grad_plan; out[DAD_VG_INTS].
inline int violation_grad_plan_report(int state_dim, int observation_dim, int action_dim, int batch, int horizon, int form,
                                      int32_t* out) {
    int D = 0;
    ViolationGradPlan q;
    const int rc = violation_grad_plan_checked(state_dim, observation_dim, action_dim, batch, horizon, form, D, q);
    if (rc != DAD_OK) return rc;
    const auto i32 = [](size_t v) { return (int32_t)std::min<size_t>(v, INT32_MAX); };
    out[DAD_VG_FORM] = q.form;
    out[DAD_VG_FWD_ROWS_PER_BLOCK] = q.fwd.rows_per_block; out[DAD_VG_FWD_GX] = (int32_t)q.fwd.gx; out[DAD_VG_FWD_GY] = (int32_t)q.fwd.gy;
    out[DAD_VG_FWD_LDS_BYTES] = i32(q.fwd.lds_bytes); out[DAD_VG_FWD_SUM_GX] = (int32_t)q.fwd.tail_gx;
    out[DAD_VG_BWD_ROWS_PER_BLOCK] = q.bwd.rows_per_block; out[DAD_VG_BWD_GX] = (int32_t)q.bwd.gx; out[DAD_VG_BWD_GY] = (int32_t)q.bwd.gy;
    out[DAD_VG_BWD_LDS_BYTES] = i32(q.bwd.lds_bytes); out[DAD_VG_BWD_SCATTER_GX] = (int32_t)q.bwd.tail_gx;
    out[DAD_VG_WORKSPACE_BYTES] = i32(q.workspace_bytes);
    out[DAD_VG_REFUSED] = q.refused;
    return DAD_OK;
}

// dad_debug_guide_plan: plan_guide for this net on trajectories of this shape; out[DAD_GD_INTS].
inline int guide_plan_report(int in_dim, const int32_t* widths, int n_layers, int activation, int batch, int horizon, int td,
                             int32_t* out) {
    const int rc = guide_shape_checked(batch, horizon, td);
    if (rc != DAD_OK) return rc;
    const GuidePlan q = plan_guide(in_dim, widths, n_layers, activation, batch, horizon, td);
    out[DAD_GD_LAYERS] = n_layers;
    out[DAD_GD_PADDED_IN] = q.padded[0]; out[DAD_GD_PADDED_1] = q.padded[1];
    out[DAD_GD_PADDED_2] = q.padded[2]; out[DAD_GD_PADDED_3] = q.padded[3];
    out[DAD_GD_ROWS_PER_BLOCK] = q.rows_per_block;
    out[DAD_GD_THREADS] = q.threads;
    out[DAD_GD_GX] = (int32_t)q.gx;
    out[DAD_GD_LDS_BYTES] = (int32_t)std::min<size_t>(q.lds_bytes, INT32_MAX);
    out[DAD_GD_REFUSED] = q.refused;
    return DAD_OK;
}

// dad_debug_optim_plan: optim_plan written down chunk by chunk, by walking the blocks with the two functions the
// kernels walk them with.
inline int optim_plan_report(const int64_t* numel, int n, std::vector<int32_t>& r) {
    OptimPlan p;
    const int rc = optim_plan(numel, n, p);
    if (rc != DAD_OK) return rc;
    r.assign(DAD_OS_HEADER, 0);
    r[DAD_OS_CHUNK] = p.g.chunk;
    r[DAD_OS_CHUNKS] = p.g.nchunks;
    r[DAD_OS_GRID] = p.g.grid;
    r[DAD_OS_PARTIALS] = p.g.grid;
    r[DAD_OS_RECORD_INTS] = DAD_OS_REC_INTS;
    for (int b = 0; b < p.g.grid; ++b) {
        int lo, hi;
        optim_block_chunks(p.g, b, lo, hi);
        int t = (int)(std::upper_bound(p.first.begin(), p.first.end(), lo) - p.first.begin()) - 1;
        for (int c = lo; c < hi; ++c) {
            while (c >= p.first[(size_t)t + 1]) ++t;
            int64_t first;
            int32_t count;
            optim_chunk_span(p.g, c, p.first[(size_t)t], numel[t], first, count);
            int32_t* rec = new_record(r, DAD_OS_REC_INTS);
            rec[DAD_OS_REC_TENSOR] = t; rec[DAD_OS_REC_FIRST] = (int32_t)(first & 0x7fffffff); rec[DAD_OS_REC_FIRST_HI] = (int32_t)(first >> 31);
            rec[DAD_OS_REC_COUNT] = count; rec[DAD_OS_REC_BLOCK] = b;
        }
    }
    return DAD_OK;
}

}  // namespace dadhost
