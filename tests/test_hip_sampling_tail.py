"""The tail of a sampling step on every path it can take, against float64.

The tail is what dad_denoise_step runs behind the convs: final_posterior_kernel (csrc/pointwise.hpp) or, on the small-batch
route, final_cc_kernel (csrc/conv_cc.hpp) -- the 1x1 output conv, the posterior mean, the guide axpy, the noise and the
inpainting --, the in-kernel Philox draws, and the three projection forms behind dad_project / dad_projection_violation
(project_kernel<1,16>, project_kernel<4,16>, project_gemm_kernel).  Structure of tests/test_hip_forward_paths.py:

(a) test_matrix_reaches_every_tail_path (no device): every case's path is read from the host plans
    (HipEngine.forward_plan(B, 0)["final"], ProjectionState.plan) and the matrix as a whole covers REQUIRED_FINAL /
    REQUIRED_PROJECTION: every form of gridDim.y of final_posterior_kernel (1, between 1 and the column groups, all column
    groups, raised by the LDS loop), blocks with 1, 2, 3 and 4 live columns per trip and several trips, a partly filled row
    tile, a padded horizon; final_cc_kernel with one and several column ranges (of unequal length; capped by 256 / batch);
    each projection form with a partly filled last block, D off the multiples of 32 and 64, D < 64, zero-padded observation
    channels, the violation, and the refusal.  The option cases cover all pairs of their six options on both kernels.
(b) test_tail_step_vs_float64 (gpu): one denoise_step per case.  eps_out against oracle.denoiser.unet_forward in float64
    (TOL_STEP; at the large batches on SUBSET samples); mean_out and the new x against the posterior formula in float64 ON
    THE KERNEL'S OWN eps_out, every element, at the forward error bound of the kernel's operation sequence
    (posterior_reference); the exact properties (inpainting, t == 0, update_x=False, a guide of weight 0, a second call).
    test_fp32_reference_is_inside_the_posterior_bound (no device) holds the bound to its condition: the same formula in
    fp32 torch, in the reference's operation order, lies inside it on every case.
(c) test_inkernel_noise_is_the_filled_noise (gpu): a step that draws its noise in the kernel equals the step on
    fill_normal's tensor of the same (seed, row_offset, draw), on both kernels; test_fill_normal_high_words (gpu): fill_normal
    against oracle.philox.normal where the high words of the block index, the draw and the seed are live.
(d) test_projection_forms_vs_float64 (gpu): every projection case against oracle.projection.apply_projection in float64,
    at alpha 1, 0.6 and 1e-3, and the violation against the float64 restatement of ProjectionLoss.compute before its mean;
    x sits inside a buffer of sentinels that must survive.

At t = T - 1 of the cosine schedule sqrt(1 / abar) is 1284: with predict_epsilon every x0 clamps there, so the option cases
that must straddle the clamp ("some, but not all") sit at t = 0 / 1 or predict x0 directly; the geometry cases run the
defaults (predict_epsilon, clip_denoised) with a guide at t = 1 and t = T - 1.

Measured on an MI355X (`-m gpu -s` prints every case; 2 s for the file's 48 GPU tests): eps_out 3.7e-7 .. 1.3e-6 from the
float64 forward (the worst at dim 512); error / bound of mean_out at most 0.86 (post_opt_pe0_clip0_t1_rows_x_g0), of x at most
0.69, where fp32 torch itself reaches 0.83 of the bound; fill_normal 2.4e-7 .. 4.8e-7 from its oracle with every high word
live; projection 2.0e-7 .. 1.3e-6 from float64 (the worst: the GEMM form with od > n), the violation 1.1e-7 x the largest of
its batch.  No case failed on the library as it was.  Deliberate one-line errors in scratch builds and what they made fail:
DESIGN.md, "Sampling tail census".
"""
import functools
import math
import time

import numpy as np
import pytest
import torch

from tests import forward_census as census
from tests.test_hip_parity import TOL_STEP, dev  # noqa: F401  (dev: fixture)
from tests.util import as_torch, max_abs

T = census.T
JG, JB, FINAL_COLS = 8, 4, 32           # final_posterior_kernel: column groups of 8, 4 columns per trip, 32 positions
CC_THREADS = 512                        # final_cc_kernel
TOL_PROJ = 2e-5                         # tests/test_hip_extra.py::test_projection_as_a_gemm_at_wide_dims
TOL_PHILOX = 2e-5                       # tests/test_hip_extra.py::test_inkernel_philox_matches_its_oracle
GUIDE_WEIGHT = 0.7
LAST = T - 1

# ------------------------------------------------------------------------------------------------ the cases
# One level (dim_mults (1,)), kernel_size 5: the conv cost is irrelevant here.  Sizes found with the host planner.
# (id, td, dim, horizon, batch, debug options, predict_epsilon, clip_denoised, t, condition, guide, outputs, features)
#   condition: "none" / "shared" (1, td) / "rows" (B, td);  outputs: "x" alone / "side" (mean_out, eps_out) / "noup" (update_x=False)
POST, CC = "final_posterior_kernel", "final_cc_kernel"
GEOMETRY_CASES = [
    ("post_td6_B1101_gy1", 6, 32, 8, 1101, {}, 1, 1, LAST, "shared", 1, "side",
     [POST, "gy==1", ("live", 1), "part_row_tile"]),
    ("post_td12_B1101_gy1", 12, 32, 8, 1101, {}, 1, 1, 1, "none", 1, "side",
     [POST, "gy==1", ("live", 2), "part_row_tile"]),
    ("post_td20_B1101_gy1", 20, 32, 8, 1101, {}, 1, 1, 1, "rows", 1, "side",
     [POST, "gy==1", ("live", 3), "part_row_tile"]),
    ("post_td67_B1101_gy1", 67, 32, 8, 1101, {}, 1, 1, 1, "shared", 1, "side",
     [POST, "gy==1", ("live", 4), ("live", 1), "trips>=2", "part_row_tile"]),
    ("post_td67_B501_gy4", 67, 32, 8, 501, {}, 1, 1, 1, "shared", 1, "side",
     [POST, "1<gy<col_groups", ("live", 3), ("live", 2), "part_row_tile"]),
    ("post_td67_B301_gy6", 67, 32, 8, 301, {}, 1, 1, LAST, "rows", 1, "side",
     [POST, "1<gy<col_groups", ("live", 2), ("live", 1), "part_row_tile"]),
    ("post_td67_d512_B1101_lds", 67, 512, 8, 1101, {}, 1, 1, 1, "shared", 1, "side",
     [POST, "gy>lds", "1<gy<col_groups", ("live", 4), ("live", 1), "trips>=2", "part_row_tile"]),
    ("post_td20_H24_B5_padded", 20, 32, 24, 5, {}, 1, 1, 1, "shared", 1, "side",
     [POST, "gy==col_groups", ("live", 1), "part_row_tile", "padded"]),
    ("post_td67_B70_gy9", 67, 32, 8, 70, {}, 1, 1, LAST, "none", 1, "side",
     [POST, "gy==col_groups", ("live", 1)]),
    ("cc_td6_B3_gy1", 6, 32, 8, 3, {}, 1, 1, 1, "shared", 1, "side",
     [CC, "cc_gy==1"]),
    ("cc_td67_B3_gy2", 67, 32, 8, 3, {}, 1, 1, LAST, "rows", 1, "side",
     [CC, "cc_gy>1_unequal"]),
    ("cc_td67_H32_B2_gy5", 67, 32, 32, 2, {}, 1, 1, 1, "shared", 1, "side",
     [CC, "cc_gy>1_unequal"]),
    ("cc_td67_H32_B100_capped", 67, 32, 32, 100, {"cc_max_rows": 4096}, 1, 1, 1, "none", 1, "side",
     [CC, "cc_gy_capped", "cc_gy>1_unequal"]),
]
# all pairs of (predict_epsilon, clip_denoised, t, condition, outputs, guide), but predict_epsilon with clip_denoised at
# t = T - 1 (module docstring), on both kernels: batch 70 takes final_posterior_kernel, batch 3 final_cc_kernel
OPTION_ROWS = [
    (0, 1, 0, "none", "x", 1),
    (1, 0, 0, "shared", "side", 1),
    (1, 0, 0, "rows", "noup", 0),
    (1, 1, 1, "none", "side", 0),
    (0, 1, 1, "shared", "noup", 1),
    (0, 0, 1, "rows", "x", 0),
    (0, 0, LAST, "none", "noup", 1),
    (1, 0, LAST, "shared", "x", 0),
    (0, 1, LAST, "rows", "side", 1),
    (1, 1, 0, "rows", "x", 1),
]
OPTION_DOMAINS = ((0, 1), (0, 1), (0, 1, LAST), ("none", "shared", "rows"), ("x", "side", "noup"), (0, 1))


def _option_cases(kernel, B):
    short = "post" if kernel == POST else "cc"
    return [(f"{short}_opt_pe{pe}_clip{clip}_t{t}_{cond}_{out}_g{g}", 6, 32, 8, B, {}, pe, clip, t, cond, g, out, [kernel])
            for pe, clip, t, cond, out, g in OPTION_ROWS]


OPTION_CASES = _option_cases(POST, 70) + _option_cases(CC, 3)
FINAL_CASES = GEOMETRY_CASES + OPTION_CASES
GAIN = {True: 1.5, False: 1.0}          # option nets: a wider output, so that predicting x0 straddles the clamp too

REQUIRED_FINAL = [POST, CC, "gy==1", "1<gy<col_groups", "gy==col_groups", "gy>lds", ("live", 1), ("live", 2), ("live", 3),
                  ("live", 4), "trips>=2", "part_row_tile", "padded", "cc_gy==1", "cc_gy>1_unequal", "cc_gy_capped"]

# (id, n, od, m, horizon, batch, scratch for the GEMM form, violation, features)
PROJECTION_CASES = [
    ("row1_D52_B3", 4, 4, 2, 8, 3, True, False, ["row1", "D<64", "D%64", "D%32"]),
    ("row1_D52_B3_violation", 4, 4, 2, 8, 3, True, True, ["row1", "D<64", "violation"]),
    ("row1_D52_B5_od6", 4, 6, 2, 8, 5, True, False, ["row1", "D<64", "od>n"]),
    ("row1_D196_B7", 4, 4, 2, 32, 7, True, False, ["row1", "D%64", "D%32"]),
    ("row1_D514_B45_noscratch", 4, 4, 2, 85, 45, False, False, ["row1", "D%64", "D%32"]),
    ("row4_D52_B515", 4, 4, 2, 8, 515, True, False, ["row4", "part_block", "D%64", "D%32"]),
    ("row4_D196_B513_violation", 4, 4, 2, 32, 513, True, True, ["row4", "part_block", "violation", "D%64", "D%32"]),
    ("row4_D52_B514_od6", 4, 6, 2, 8, 514, True, False, ["row4", "part_block", "od>n"]),
    ("gemm_D514_B45", 4, 4, 2, 85, 45, True, False, ["gemm", "part_block", "D%64", "D%32"]),
    ("gemm_D514_B33_od6", 4, 6, 2, 85, 33, True, False, ["gemm", "part_block", "od>n", "D%64", "D%32"]),
]
REQUIRED_PROJECTION = [(f, g) for f in ("row1", "row4", "gemm") for g in ("D%64", "D%32")] + \
                      [("row4", "part_block"), ("gemm", "part_block"), ("row1", "D<64"), ("row1", "od>n"), ("gemm", "od>n"),
                       ("row1", "violation"), ("row4", "violation")]
ALPHAS = (1.0, 0.6, 1e-3)


# ------------------------------------------------------------------------------------------------ (a)
def live_columns(td, gy):
    """Per block row `by` of final_posterior_kernel, the live-column count of each of its trips: the kernel walks
    jb = by * JG, by * JG + JB * JG * gy, ... < td and runs final_dots<min(JB, (td - 1 - jb) / (JG * gy) + 1)>."""
    jstep = JG * gy
    return [[min(JB, (td - 1 - jb) // jstep + 1) for jb in range(by * JG, td, JB * jstep)] for by in range(gy)]


def final_features(case, plan, padded):
    _, td, dim, H, B = case[:5]
    gx, gy, kernel = plan["final"]
    out = {kernel}
    if kernel == POST:
        row_tiles = (B * H + FINAL_COLS - 1) // FINAL_COLS
        col_groups = (td + JG - 1) // JG
        assert gx == row_tiles and 1 <= gy <= col_groups
        out.add("gy==1" if gy == 1 else "1<gy<col_groups" if gy < col_groups else "gy==col_groups")
        if gy > max(1, min(col_groups, 512 // row_tiles)):
            out.add("gy>lds")
        trips = live_columns(td, gy)
        out |= {("live", n) for by in trips for n in by}
        if max(len(by) for by in trips) >= 2:
            out.add("trips>=2")
        if (B * H) % FINAL_COLS:
            out.add("part_row_tile")
        if padded:
            out.add("padded")
    else:
        want = (H * td + CC_THREADS - 1) // CC_THREADS
        assert gx == B and gy == max(1, min(want, td, 256 // B)) and not padded
        out.add("cc_gy==1" if gy == 1 else "cc_gy>1")
        if gy > 1 and td % gy:
            out.add("cc_gy>1_unequal")          # ranges [td by / gy, td (by + 1) / gy) of two lengths
        if gy == 256 // B < min(want, td):
            out.add("cc_gy_capped")
    return out


def _final_plan(case):
    _, td, dim, H, B, options = case[:6]
    eng = census.host_engine(td, dim, (1,), H, 5, "fp32")
    census.set_options(eng, -1, options)
    return eng.forward_plan(B, 0), bool(eng.rows_padded)


def projection_features(case, plan):
    _, n, od, m, H, B, scratch, violation, _ = case
    D = (H + 1) * n + H * m
    out = {plan["form"]}
    if B % plan["rows_per_block"]:
        out.add("part_block")
    out |= {name for name, on in (("D%64", D % 64), ("D%32", D % 32), ("D<64", D < 64), ("od>n", od > n),
                                  ("violation", violation)) if on}
    return out


def _projection_plan(case):
    from dynamics_aware_diffusion_amd._engine import ProjectionState
    _, n, od, m, H, B, scratch, violation, _ = case
    return ProjectionState.host(n, od, m, gemm=scratch).plan(B, H, violation=violation)


def test_matrix_reaches_every_tail_path():
    from dynamics_aware_diffusion_amd._engine import ProjectionState
    assert len({c[0] for c in FINAL_CASES}) == len(FINAL_CASES)
    reached = set()
    for case in FINAL_CASES:
        have = final_features(case, *_final_plan(case))
        missing = [f for f in case[-1] if f not in have]
        assert not missing, f"{case[0]}: the planner no longer takes this case through {missing}; it has {sorted(map(str, have))}"
        reached |= have
    missing = [f for f in REQUIRED_FINAL if f not in reached]
    assert not missing, f"no case of the matrix reaches {missing}"
    # final_cc_kernel stages whole samples of the real horizon: the small-batch plan admits no padded horizon
    for td in (6, 67):
        eng = census.host_engine(td, 32, (1,), 24, 5, "fp32")
        assert eng.rows_padded
        for B in range(1, 22):
            plan = eng.forward_plan(B, 0)
            assert not plan["small"] and plan["final"][2] == POST, (td, B)
    # the option cases: all pairs on both kernels (but predict_epsilon and clip_denoised at t = T - 1)
    for i in range(6):
        for j in range(i + 1, 6):
            want = {(a, b) for a in OPTION_DOMAINS[i] for b in OPTION_DOMAINS[j]}
            assert {(r[i], r[j]) for r in OPTION_ROWS} == want, (i, j)
    assert not [r for r in OPTION_ROWS if r[0] and r[1] and r[2] == LAST]
    # projection
    assert len({c[0] for c in PROJECTION_CASES}) == len(PROJECTION_CASES)
    reached = set()
    for case in PROJECTION_CASES:
        plan = _projection_plan(case)
        assert not plan["refused"], case[0]
        have = projection_features(case, plan)
        missing = [f for f in case[-1] if f not in have]
        assert not missing, f"{case[0]}: dad_project no longer takes this case through {missing}; it has {sorted(have)} ({plan})"
        B, rb = case[5], plan["rows_per_block"]
        assert plan["grid"][0] == (B + rb - 1) // rb
        reached |= {(plan["form"], f) for f in have}
    missing = [f for f in REQUIRED_PROJECTION if f not in reached]
    assert not missing, f"no projection case reaches {missing}"
    # the rules of the dispatch, at their thresholds (D = 6 H + 4 for n = 4, m = 2)
    st, bare = ProjectionState.host(4, 4, 2), ProjectionState.host(4, 4, 2, gemm=False)
    assert st.plan(512, 32)["form"] == "row1" and st.plan(513, 32)["form"] == "row4"               # batch > 512
    assert st.plan(32, 84)["form"] == "row1" and st.plan(32, 85)["form"] == "gemm"                 # D >= 512 (508 / 514)
    assert st.plan(31, 85)["form"] == "row1" and bare.plan(32, 85)["form"] == "row1"               # batch >= 32, scratch
    assert st.plan(513, 85, violation=True)["form"] == "row4" and st.plan(513, 85)["form"] == "gemm"    # never the violation
    assert st.plan(513, 100)["form"] == "gemm" and st.plan(513, 100, violation=True)["form"] == "row1"  # 4 rows of D = 604: 164 KB
    assert st.plan(513, 99, violation=True)["form"] == "row4"                                           # D = 598: 163 KB
    # one trajectory's partial sums: 17 D floats fit 160 KB up to D = 2409 (H = 400: D = 2404, H = 401: D = 2410)
    assert not bare.plan(3, 400)["refused"] and bare.plan(3, 401)["refused"] and bare.plan(600, 401)["refused"]
    assert st.plan(31, 401)["refused"] and st.plan(32, 401, violation=True)["refused"]
    big = st.plan(32, 401)
    assert big["form"] == "gemm" and not big["refused"] and big["grid"] == (1, (2410 + 31) // 32)


# ------------------------------------------------------------------------------------------------ (b)
U = 2.0 ** -24                          # unit roundoff of fp32
ULP = 2.0 ** -23


def posterior_reference(sched, t, x, eps, z, g, guide_weight, cond, predict_epsilon, clip_denoised):
    """The posterior of diffusion.py:159-223 / policies.py:84-110 in float64 on a given network output, and the forward
    error bound of the kernel's evaluation of it (`finish` of final_posterior_kernel; final_cc_kernel runs the same lines).

    sched: the model's fp32 buffers; x, eps, z, g: float64 arrays (B, H, td); cond None, (1, td) or (B, td).
    Returns (mean, x_new, bound of mean_out, bound of the new x, how many x0 lie inside the clamp).

    The bound: every rounded fp32 operation contributes u |its exact result|, u = 2^-24, and errors already made travel
    through the operations behind them (standard forward analysis; u / (1 - 16 u) for u pays the second-order terms of the
    at most 16 roundings of one output).  An fma is counted as the two roundings of its mul and add, so a contracted and an
    uncontracted build are both inside.  Operation by operation:
        a = c_recip x, b = c_recipm1 eps, x0 = a - b          u (|a| + |b| + |x0|)        [predict_epsilon; else x0 = eps, exact]
        x0 = clamp(x0, -1, 1)                                 1-Lipschitz: the bound of x0 stands
        c = coef1 x0, d = coef2 x, mean = c + d               coef1 e(x0) + u (|c| + |d| + |mean|)
        gs = weight expf(lv), q = gs g, mean = mean + q       (2 u + 2 ulp) |q| + u |mean|: the two products, the sum, and two
                                                              ulps (2^-23 each) of q because the host's expf is not exp
        s = sigma z, x = mean + s                             e(mean) + (u + 2 ulp) |s| + u |x|: likewise for sigma = expf(lv / 2)
                                                              (lv / 2 is exact); sigma = 0 at t = 0: x = mean exactly
    Inpainted rows are copies: bound 0."""
    cr, cm, c1, c2, lv = (float(sched[k][t]) for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                       "posterior_mean_coef1", "posterior_mean_coef2",
                                                       "posterior_log_variance_clipped"))
    u = U / (1.0 - 16.0 * U)
    if predict_epsilon:
        a, b = cr * x, cm * eps
        x0 = a - b
        e0 = u * (np.abs(a) + np.abs(b) + np.abs(x0))
    else:
        x0, e0 = eps.copy(), np.zeros_like(eps)
    unclamped = int((np.abs(x0) < 1.0).sum())
    if clip_denoised:
        x0 = np.clip(x0, -1.0, 1.0)
    c, d = c1 * x0, c2 * x
    mean = c + d
    em = c1 * e0 + u * (np.abs(c) + np.abs(d) + np.abs(mean))
    w32 = float(np.float32(guide_weight))
    if g is not None and w32 > 0.0:
        q = (w32 * math.exp(lv)) * g
        mean = mean + q
        em = em + (2.0 * u + 2.0 * ULP) * np.abs(q) + u * np.abs(mean)
    s = (0.0 if t == 0 else math.exp(0.5 * lv)) * z
    xn = mean + s
    ex = em + (u + 2.0 * ULP) * np.abs(s) + u * np.abs(xn)
    if cond is not None:
        xn[:, 0], ex[:, 0] = cond, 0.0
    return mean, xn, em, ex, unclamped


def posterior_fp32(sched, t, x, eps, z, g, guide_weight, cond, predict_epsilon, clip_denoised):
    """The same formula by torch in fp32, in the reference's operation order (oracle.denoiser.p_mean_variance /
    denoise_step behind the network).  Returns (mean, x_new)."""
    cr, cm, c1, c2, lv = (sched[k][t] for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                "posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped"))
    x0 = cr * x - cm * eps if predict_epsilon else eps
    if clip_denoised:
        x0 = torch.clamp(x0, -1.0, 1.0)
    mean = c1 * x0 + c2 * x
    if g is not None and guide_weight > 0:
        mean = mean + guide_weight * lv.exp() * g
    xn = mean + (0.0 if t == 0 else 1.0) * torch.exp(0.5 * lv) * z
    if cond is not None:
        xn[:, 0] = cond
    return mean, xn


def _ratio(err, bound):
    """Largest err / bound; an error where the bound is 0 (copies) is infinite."""
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _inputs(case):
    """x, z, guide gradient, condition of a case (fp32 numpy; the condition None, (1, td) or (B, td))."""
    from dynamics_aware_diffusion_amd.utils import synth
    name, td, dim, H, B = case[:5]
    cond_kind = case[9]
    x = synth.normal_like(31, f"tail.x.{name}", (B, H, td))
    z = synth.normal_like(31, f"tail.z.{name}", (B, H, td))
    g = synth.normal_like(31, f"tail.g.{name}", (B, H, td))
    cond = None if cond_kind == "none" else synth.uniform(31, f"tail.c.{name}", (1 if cond_kind == "shared" else B, td), 0.9)
    return x, z, g, cond


def _schedule():
    from dynamics_aware_diffusion_amd.models.diffusion import make_schedule
    return make_schedule("cosine", T)


@pytest.mark.parametrize("case", FINAL_CASES, ids=lambda c: c[0])
def test_fp32_reference_is_inside_the_posterior_bound(case):
    """The condition of the bound: a correct fp32 evaluation is inside it, on the shapes and options of every case (the
    first 16 samples; a synthetic network output of the spread the nets have, so that the clamp is straddled)."""
    from dynamics_aware_diffusion_amd.utils import synth
    name, td, dim, H, B, _, pe, clip, t, cond_kind, guide, _, _ = case
    sched = _schedule()
    x, z, g, cond = (None if v is None else v[:16] for v in _inputs(case))
    eps = (0.6 * synth.normal_like(31, f"tail.eps.{name}", x.shape)).astype(np.float32)
    gw = GUIDE_WEIGHT if guide else 0.0
    mean64, xn64, em, ex, _ = posterior_reference(sched, t, x.astype(np.float64), eps.astype(np.float64), z.astype(np.float64),
                                                 g.astype(np.float64), gw, cond, pe, clip)
    tt = lambda v: None if v is None else torch.from_numpy(v)
    mean32, xn32 = posterior_fp32(sched, t, tt(x), tt(eps), tt(z), tt(g), gw, tt(cond), pe, clip)
    r_mean = _ratio(np.abs(mean32.numpy().astype(np.float64) - mean64), em)
    r_x = _ratio(np.abs(xn32.numpy().astype(np.float64) - xn64), ex)
    print(f"\n{name}: fp32 torch vs float64, error / bound: mean {r_mean:.3f}, x {r_x:.3f}")
    assert r_mean <= 1.0 and r_x <= 1.0


def subset(B, H):
    """At most 16 samples: the first, the last, and those either side of a row-tile boundary (tiles of FINAL_COLS
    positions), near the front, in the middle and at the last tile."""
    if B <= 16:
        return list(range(B))
    per = max(1, FINAL_COLS // H)
    mid, last = (B // 2) // per * per, (B - 1) // per * per
    picks = {0, 1, per - 1, per, per + 1, mid - 1, mid, mid + 1, last - 1, last, B - 2, B - 1}
    return sorted(s for s in picks if 0 <= s < B)


@functools.lru_cache(maxsize=None)
def _net(td, dim, option_net):
    from dynamics_aware_diffusion_amd.utils import synth
    return synth.synth_unet_state(td, dim, (1,), seed=47, affine_jitter=0.3, gain=GAIN[option_net])


@functools.lru_cache(maxsize=None)
def _eps64(name):
    """The float64 forward of a case on its SUBSET samples; nobody writes into it."""
    from oracle import denoiser as orc
    case = next(c for c in FINAL_CASES if c[0] == name)
    _, td, dim, H, B, _, _, _, t = case[:9]
    w64 = orc.cast_weights(as_torch(_net(td, dim, "_opt_" in name)), torch.float64)
    rows = subset(B, H)
    x = torch.from_numpy(_inputs(case)[0][rows]).double()
    with torch.no_grad():
        return rows, orc.unet_forward(w64, x, torch.full((len(rows),), t, dtype=torch.long)).numpy()


_DIFFUSIONS = {}


def _diffusion(case, dev):
    from tests.test_hip_long_horizon import _diffusion as build
    name, td, dim, H, _, _, pe, clip = case[:8]
    key = (td, dim, H, pe, clip, "_opt_" in name)
    if key not in _DIFFUSIONS:
        if len(_DIFFUSIONS) > 3:
            _DIFFUSIONS.clear()
        _DIFFUSIONS[key] = build(td, td - 1, 1, dim, (1,), H, T, _net(td, dim, key[-1]), dev,
                                 predict_epsilon=bool(pe), clip_denoised=bool(clip))
    return _DIFFUSIONS[key]


@pytest.fixture(scope="module", autouse=True)
def _file_seconds():
    t0 = time.perf_counter()
    yield
    print(f"\ntests/test_hip_sampling_tail.py: {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("case", FINAL_CASES, ids=lambda c: c[0])
def test_tail_step_vs_float64(case, dev):
    from tests.test_hip_forward_paths import _apply
    name, td, dim, H, B, options, pe, clip, t, cond_kind, guide, outputs, features = case
    diff = _diffusion(case, dev)
    eng = diff._engine(dev)
    x_h, z_h, g_h, cond_h = _inputs(case)
    x, z, g = (torch.from_numpy(v).to(dev) for v in (x_h, z_h, g_h))
    cond = None if cond_h is None else torch.from_numpy(cond_h).to(dev)
    gw = GUIDE_WEIGHT if guide else 0.0
    kw = dict(noise=z, cond0=cond, guide_grad=g if guide else None, guide_weight=gw)

    def step(update_x=True, side=True, **over):
        xs = x.clone()
        mean, eps = (torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))) if side else (None, None)
        eng.denoise_step(xs, t, **{**kw, **over}, mean_out=mean, eps_out=eps, update_x=update_x)
        return xs, mean, eps

    try:
        _apply(eng, -1, options, diff.model.small_batch_kernels)
        plan = eng.forward_plan(B, 0)
        have = final_features(case, plan, bool(eng.rows_padded))
        assert not [f for f in features if f not in have], (name, plan["final"])
        xa, mean_a, eps_a = step()
        xb, mean_b, eps_b = step()
        # the outputs the case asks for, and the exact properties
        if outputs == "x":
            xo, _, _ = step(side=False)
            assert torch.equal(xo, xa), "x alone differs from x with the side outputs"
        elif outputs == "noup":
            xo, mean_o, eps_o = step(update_x=False)
            assert torch.equal(xo, x), "update_x=False wrote x"
            assert torch.equal(mean_o, mean_a) and torch.equal(eps_o, eps_a)
        if guide:
            x0g, mean_0g, _ = step(guide_grad=None, guide_weight=0.0)
            xw0, mean_w0, _ = step(guide_weight=0.0)
        else:
            x0g, mean_0g = xa, mean_a
            xw0, mean_w0, _ = step(guide_grad=g, guide_weight=0.0)
        assert diff.model._engine is eng
    finally:
        _apply(eng, -1, {}, diff.model.small_batch_kernels)
    torch.cuda.synchronize()
    assert torch.equal(xa, xb) and torch.equal(mean_a, mean_b) and torch.equal(eps_a, eps_b), "a second call gives other bits"
    assert torch.equal(xw0, x0g) and torch.equal(mean_w0, mean_0g), "a guide gradient of weight 0 changed bits"
    if cond is not None:
        assert torch.equal(xa[:, 0], cond.expand(B, td)), "inpainted rows are not the condition"
    if t == 0:
        free = slice(1, None) if cond is not None else slice(None)
        assert torch.equal(xa[:, free], mean_a[:, free]), "t == 0: x is not mean_out"
    xa, mean_a, eps_a = (v.cpu().numpy() for v in (xa, mean_a, eps_a))
    assert np.isfinite(xa).all() and np.isfinite(mean_a).all() and np.isfinite(eps_a).all()
    # 1. eps_out against the float64 forward
    rows, eps64 = _eps64(name)
    e_eps = max_abs(eps_a[rows], eps64)
    # 2. mean_out and x against the posterior formula on the kernel's own eps_out
    sched = {k: v.detach().cpu() for k, v in diff.named_buffers()}        # the model's own fp32 schedule
    mean64, xn64, em, ex, unclamped = posterior_reference(sched, t, x_h.astype(np.float64), eps_a.astype(np.float64),
                                                          z_h.astype(np.float64), g_h.astype(np.float64), gw, cond_h, pe, clip)
    r_mean, r_x = _ratio(np.abs(mean_a - mean64), em), _ratio(np.abs(xa - xn64), ex)
    print(f"\n{name}: grid {plan['final']}: eps_out vs float64 on {len(rows)} samples {e_eps:.2e}; error / bound of mean_out "
          f"{r_mean:.3f} (max |error| {max_abs(mean_a, mean64):.2e}), of x {r_x:.3f} ({max_abs(xa, xn64):.2e}); "
          f"{unclamped} of {xa.size} x0 inside the clamp")
    assert e_eps <= TOL_STEP, f"{name}: eps_out {e_eps:.2e} from the float64 forward"
    assert r_mean <= 1.0, f"{name}: mean_out {r_mean:.3f} x the forward error bound from the float64 posterior of its eps_out"
    assert r_x <= 1.0, f"{name}: x {r_x:.3f} x the forward error bound from the float64 posterior of its eps_out"
    if clip and "_opt_" in name:
        assert 0 < unclamped < xa.size, f"{name}: the inputs do not straddle the clamp ({unclamped} of {xa.size} inside)"


# ------------------------------------------------------------------------------------------------ (c)
NOISE_CASES = [
    # (case of the matrix, seed, row_offset, draw)
    ("cc_td6_B3_gy1", 5, 0, 1),
    ("cc_td67_B3_gy2", 0xDEADBEEF12345678, (1 << 27) + 3, (1 << 32) + 1),
    ("post_opt_pe1_clip0_t19_shared_x_g0", 7, 11, 3),
    ("post_td67_B501_gy4", 0xDEADBEEF12345678, (1 << 27) + 3, (1 << 32) + 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("noise_case", NOISE_CASES, ids=lambda c: c[0])
def test_inkernel_noise_is_the_filled_noise(noise_case, dev):
    """denoise_step(seed, row_offset, draw) equals denoise_step(noise=fill_normal(seed, row_offset, draw)) bit for bit: the
    device function is the same, so this pins the element index and the offset plumbing of both kernels."""
    name, seed, row_offset, draw = noise_case
    case = next(c for c in FINAL_CASES if c[0] == name)
    _, td, dim, H, B = case[:5]
    diff = _diffusion(case, dev)
    eng = diff._engine(dev)
    assert final_features(case, eng.forward_plan(B, 0), bool(eng.rows_padded)) >= set(case[-1])
    x = torch.from_numpy(_inputs(case)[0]).to(dev)
    z = torch.empty_like(x)
    eng.fill_normal(z, seed, row_offset=row_offset, draw=draw)
    drawn, given, other = x.clone(), x.clone(), x.clone()
    eng.denoise_step(drawn, LAST, seed=seed, row_offset=row_offset, draw=draw)
    eng.denoise_step(given, LAST, noise=z)
    eng.denoise_step(other, LAST, seed=seed, row_offset=row_offset, draw=draw + 1)
    torch.cuda.synchronize()
    assert torch.isfinite(z).all() and 0.8 < float(z.std()) < 1.2
    assert torch.equal(drawn, given), f"{name}: the kernel's own draws are not fill_normal's"
    assert not torch.equal(drawn, other)


@pytest.mark.gpu
def test_fill_normal_high_words(dev):
    """fill_normal against oracle.philox.normal where the high words are live: an element offset of 3 x 2^33 (the Philox
    block index is beyond 2^32), a draw beyond 2^32, a seed with a high word."""
    from dynamics_aware_diffusion_amd._engine import HipEngine
    from oracle import philox
    eng = HipEngine(transition_dim=6, dim=32, channels=(32,), horizon=32, n_timesteps=T, device=dev)
    B, E = 5, 32 * 6
    for seed, row_offset, draw in ((1, 1 << 27, 0), (1, 3, (1 << 32) + 5), (0xDEADBEEF12345678, 3, 2),
                                   (0xDEADBEEF12345678, (1 << 27) + 3, (1 << 32) + 5)):
        x = torch.empty(B, 32, 6, device=dev)
        eng.fill_normal(x, seed, row_offset=row_offset, draw=draw)
        first = row_offset * E
        idx = np.arange(B * E, dtype=np.uint64) + np.uint64(first)
        assert row_offset < (1 << 27) or int(idx[0]) >> 2 >= 1 << 32
        want = philox.normal(idx, draw, seed).reshape(B, 32, 6)
        err = max_abs(x.cpu().numpy(), want)
        # the low words alone give other numbers
        low = philox.normal(idx & np.uint64(0x3FFFFFFFF), draw & 0xFFFFFFFF, seed & 0xFFFFFFFF).reshape(B, 32, 6)
        print(f"\nfill_normal seed {seed:#x} row_offset {row_offset} draw {draw}: |hip - oracle| {err:.2e}")
        assert err <= TOL_PHILOX
        assert max_abs(want, low) > 0.5


# ------------------------------------------------------------------------------------------------ (d)
@functools.lru_cache(maxsize=None)
def _projector(n, od, m, H):
    """A projector of rank n + H m, normaliser statistics and their float64 copies; nobody writes into it."""
    from dynamics_aware_diffusion_amd.utils import synth
    D = (H + 1) * n + H * m
    Q, _ = np.linalg.qr(np.random.default_rng(13).normal(size=(D, n + H * m)))
    P = torch.from_numpy((Q @ Q.T).astype(np.float32))
    stats = [torch.from_numpy(v) for v in (synth.normal_like(8, "tail.om", (od,)), 1.0 + synth.uniform(8, "tail.os", (od,), 0.5),
                                           synth.normal_like(8, "tail.am", (m,)), 1.0 + synth.uniform(8, "tail.as", (m,), 0.5))]
    return P, stats


def _violation64(x, P, n, od, stats):
    """ProjectionLoss.compute (losses/__init__.py:161-186) before its mean, per row, in float64 (od == n there)."""
    om, osd, am, asd = (s.double() for s in stats)
    s = x[:, :, :od] * osd + om
    a = x[:, :, od:] * asd + am
    v = torch.cat([torch.cat([s, s[:, -1:]], dim=1).reshape(x.shape[0], -1), a.reshape(x.shape[0], -1)], dim=1)
    return ((v - v @ P) ** 2).sum(dim=1)


SENTINEL = 12345.0
PAD_ROWS = 40           # more than the 32 rows of a GEMM block


@pytest.mark.gpu
@pytest.mark.parametrize("case", PROJECTION_CASES, ids=lambda c: c[0])
def test_projection_forms_vs_float64(case, dev):
    from dynamics_aware_diffusion_amd._engine import ProjectionState
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import projection as oproj
    name, n, od, m, H, B, scratch, violation, features = case
    P, stats = _projector(n, od, m, H)
    st = ProjectionState(P, *stats, n, od, m, dev)
    st.gemm = scratch
    plan = st.plan(B, H, violation=violation)
    assert not [f for f in features if f not in projection_features(case, plan)], plan
    x_h = torch.from_numpy(synth.normal_like(8, f"tail.px.{name}", (B, H, od + m)))
    buf = torch.full((PAD_ROWS + B + PAD_ROWS, H, od + m), SENTINEL, device=dev)
    x = buf[PAD_ROWS:PAD_ROWS + B]
    assert x.is_contiguous()

    def fences_stand():
        return bool((buf[:PAD_ROWS] == SENTINEL).all()) and bool((buf[PAD_ROWS + B:] == SENTINEL).all())

    om, osd, am, asd = (s.double() for s in stats)
    if violation:
        x.copy_(x_h)
        got = st.violation(x)
        again = st.violation(x)
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), x_h), "the violation wrote x"
        assert fences_stand()
        want = _violation64(x_h.double(), P.double(), n, od, stats)
        err, scale = max_abs(got.cpu().numpy(), want.numpy()), float(want.max())
        print(f"\n{name}: {plan['form']} grid {plan['grid']}: violation, max |hip - float64| {err:.2e} = {err / scale:.2e} x the largest ({scale:.3e})")
        assert err <= TOL_PROJ * scale
        assert torch.equal(got, again)
        return
    for alpha in ALPHAS:
        a32 = float(np.float32(alpha))
        want = oproj.apply_projection(x_h.double(), P.double(), a32, n, od, om[:n], osd[:n], am, asd)
        outs = []
        for _ in range(2):
            x.copy_(x_h)
            if scratch:                     # what the GEMM form does not write into its scratch copy must show
                st._check_x(x)
                st._scratch.fill_(SENTINEL)
            st.apply(x, alpha)
            torch.cuda.synchronize()
            outs.append(x.cpu())
        err = max_abs(outs[0].numpy(), want.numpy())
        print(f"\n{name}: {plan['form']} grid {plan['grid']}: alpha {alpha}: max |hip - float64| {err:.2e}")
        assert err <= TOL_PROJ, (name, alpha)
        assert torch.equal(outs[0], outs[1]), "a second call gives other bits"
        assert fences_stand(), "rows outside the batch were written"
        if od > n:
            assert bool((outs[0][:, :, n:od] == 0).all()), "observation channels beyond the state are not zero"
