"""Every kernel the backward pass can reach, run against float64.

tests/backward_census.py (a manual, host-only tool) asks HipEngine.backward_steps (dad_debug_backward_steps: everything
dad_unet_backward replays, read from its list of steps and the per-batch geometry it launches from) what a bounded space of
architectures, batches 1..512 and wgrad_blocks default / 1 / 16 / 4096 runs, and picks by greedy set cover the CASES below;
NOT_REACHED lists the registered conv_wgrad kernels nothing in that space launches ("not reached in this space", not
"dead": DESIGN.md, "Backward kernel census").  The data-gradient convs are keyed by mode 3 of
tests/test_hip_forward_paths.py and are not repeated here.

(a) test_matrix_reaches_every_backward_kernel (no device): every case's plan holds the keys the case exists for; the
    conv_wgrad instantiations the matrix launches and NOT_REACHED are disjoint and together are the 40 of
    the registry's conv_wgrad family (dad_debug_kernel_list); every launched instantiation also runs with two or more chunks in a block (the
    double-buffered steady state); a part-filled last chunk behind full ones on every tile, partly filled last M and C
    tiles, the transposed conv's swapped roles on every aligned tile windowed and not; the six GroupNorm-backward forms
    (gn_mish_bwd_wave_kernel<1 | 2 | 4 | 8 | 16>, gn_mish_bwd_kernel) each with and without the d temb store, the block form,
    <1> and <16> with a zero-padded horizon and zero-padded groups, <1> on a pair shorter than a wave; take_cols,
    row_partial_sums, the identity residual as a copy / an add / into d x / a staged CONV_UP data gradient, sum_slabs at
    2..8 slabs and beyond 8 with equal and unequal trips, col_sums_many below 25 rows / unrolled / unrolled with a tail,
    the padded-horizon copies and slice_cols.  A retuned planner that moves a case off its path fails here.
(b) test_backward_case_vs_float64 (gpu): each case builds its net with synthetic weights (GroupNorm gamma / beta and the
    biases off their defaults), asserts its keys on the step report of the engine that runs, runs one training step and
    compares with oracle.denoiser on cast_weights(w, float64): every parameter gradient and d loss / d x_t at REL =
    2e-5 max|g_f64| (scales of tests/util.py::grad_scales), the training forward's output at TOL_STEP (5e-6), the loss at
    2e-6 relative — the gates of tests/test_hip_train_batch.py, none new — and a second call bit for bit.  A case is
    admitted only if the fp32 oracle itself is within REL / 2 of float64 on every tensor (asserted; the census checks it
    on the CPU with --check-oracle), or the gate could not tell a wrong kernel from fp32.

The census (4 644 architectures, 278 640 plans, 66 866 distinct key sets, 187 keys) launches 38 of the 40 conv_wgrad
instantiations, each also in its steady state, all six GroupNorm-backward forms and every step kind; the 17 cases cover all
187 keys.  No plan of the space puts a concat boundary inside one block's staged columns (the report's `concat_inside`).

Measured on an MI355X (`-s` prints every case; 6.0 s for the file's 17 GPU cases, the whole GPU suite 10.0 minutes):
gradients 7.1e-7 .. 3.3e-6 x max|g| from float64 (worst: k5_d32_m1421_H256_td6_B1_wb1), the fp32 oracle 6.1e-7 .. 4.1e-6
(worst: the same case); training-forward outputs 3.5e-7 .. 1.1e-6 (the fp32 oracle 6.0e-7 .. 1.7e-6); losses 6e-9 .. 1.1e-7
relative.

Deliberate one-line errors (scratch builds, none committed; value errors only, no access out of bounds), each run against
this file and the new refresh test of tests/test_hip_train.py:
    conv_wgrad, WIN on the 64 x 64 tile: a window's right halo rows zero also inside the sample
        -> k3_d128_m1421_H512_td6_B1_wb1, k5_d256_m11_H384_td6_B1_wb1, k7_d256_m11_H384_td6_B1_wb1 (4.7e-2 .. 8.3e-2 x max|g|)
    conv_wgrad, 7 taps on the 64-row tiles (0 and 1): tap 5 reads tap 4's staged row
        -> k7_d48_m14_H32_td6_B3_wb1, k7_d128_m1421_H8_td6_B13_wb1, k7_d48_m14_H384_td6_B1_wb1, k7_d256_m11_H384_td6_B1_wb1 (0.6 .. 1.1)
    repack_many_kernel: the second image of a refresh skipped
        -> all six cases of test_refresh_with_changed_weights_equals_a_fresh_engine (d x differs by 1.9e-5 .. 9.2e-5)
With these three together in the library the whole earlier GPU suite (681 tests) passed: exactly the cases that launch
the forms fail, and nothing else noticed.
    gn_mish_bwd_kernel: the zero fill of the padded positions dropped
        -> k3_d64_m1421_H384_td6_B1_wb1, k7_d48_m14_H384_td6_B1_wb1, k5_d256_m11_H384_td6_B1_wb1, k7_d256_m11_H384_td6_B1_wb1
    take_cols_kernel: the second side's columns taken one quad early
        -> the six cases on the shrinking dim_mults (1, 4, 2, 1)
(the earlier suite was not run with these two: whether it notices them is not known.)
    gn_mish_bwd_wave_kernel<16>: `live` of the first pass ignoring lreal
        -> nothing fails, here or anywhere: d A is already zero on the padded positions (the data-gradient convs write zeros
           there), so that mask is redundant as the pass is built, and the second pass's own mask keeps d H zero.  The keys
           ("gn", 16, 1, ...) therefore assert that the form is launched on a padded horizon, not that this mask works.
           The same error in the second pass's mask was not run.
"""
import functools

import numpy as np
import pytest
import torch

from tests import backward_census as census
from tests.test_hip_parity import TOL_STEP, dev  # noqa: F401  (dev: fixture)
from tests.test_hip_train_batch import REL, T  # 2e-5 x max|g_f64| per tensor and 20 timesteps: that module's own
from tests.util import as_torch, grad_scales, max_abs

ADMIT = REL / 2                      # the fp32 oracle's own distance from float64 a case is admitted with
LOSS_REL = 2e-6                      # the loss gate of tests/test_hip_train_batch.py::test_large_batch_gradients_vs_float64
SEED = 47

# (id, td, dim, mults, horizon (real: the engine pads 24 / 100 / 200 / 384, and the widths of dim 48 / 96), kernel_size, batch,
#  wgrad_blocks (None: the default), keys it exists for)
CASES = [
    ('k3_d128_m1421_H8_td6_B5_wb1', 6, 128, (1, 4, 2, 1), 8, 3, 5, 1,
     [('bias',), ('cols',), ('colsums', 'short'), ('gn', 1, 1, 0, 0, 0), ('gn', 1, 1, 0, 0, 1), ('gn', 1, 1, 0, 1, 0), ('gn', 1, 1, 0, 1, 1), ('gn', 2, 1, 0, 0, 0), ('gn', 2, 1, 0, 1, 0), ('gn', 4, 1, 0, 0, 0), ('gn', 4, 1, 0, 1, 0), ('padcopy',), ('resid', 'add'), ('resid', 'copy'), ('resid', 'stage'), ('wgrad', 1, 0, 0), ('wgrad', 1, 0, 0, 'part'), ('wgrad', 1, 0, 0, 'steady'), ('wgrad', 1, 1, 0), ('wgrad', 1, 1, 0, 'part'), ('wgrad', 1, 1, 0, 'steady'), ('wgrad', 1, 2, 0), ('wgrad', 1, 3, 0), ('wgrad', 1, 3, 0, 'edge_c'), ('wgrad', 1, 3, 0, 'edge_m'), ('wgrad', 1, 3, 0, 'part'), ('wgrad', 1, 3, 0, 'steady'), ('wgrad', 3, 0, 0), ('wgrad', 3, 0, 0, 'part'), ('wgrad', 3, 0, 0, 'steady'), ('wgrad', 3, 1, 0), ('wgrad', 3, 1, 0, 'part'), ('wgrad', 3, 1, 0, 'steady'), ('wgrad', 3, 2, 0), ('wgrad', 3, 2, 0, 'part'), ('wgrad', 3, 2, 0, 'steady'), ('wgrad', 3, 3, 0), ('wgrad', 3, 3, 0, 'edge_c'), ('wgrad', 3, 3, 0, 'part'), ('wgrad', 3, 3, 0, 'steady'), ('wgrad', 4, 0, 0), ('wgrad', 4, 0, 0, 'swapped'), ('wgrad', 4, 1, 0), ('wgrad', 4, 1, 0, 'swapped'), ('wgrad', 4, 2, 0), ('wgrad', 4, 2, 0, 'part'), ('wgrad', 4, 2, 0, 'steady'), ('wgrad', 4, 2, 0, 'swapped')]),
    ('k5_d32_m1421_H256_td6_B1_wb1', 6, 32, (1, 4, 2, 1), 256, 5, 1, 1,
     [('gn', 1, 0, 0, 0, 0), ('gn', 1, 0, 0, 0, 1), ('gn', 1, 0, 0, 1, 0), ('gn', 1, 0, 0, 1, 1), ('gn', 2, 0, 0, 0, 0), ('gn', 2, 0, 0, 1, 0), ('gn', 4, 0, 0, 0, 0), ('gn', 4, 0, 0, 1, 0), ('gn', 8, 0, 0, 0, 0), ('gn', 8, 0, 0, 1, 0), ('slice_cols',), ('wgrad', 1, 3, 1), ('wgrad', 1, 3, 1, 'edge_c'), ('wgrad', 1, 3, 1, 'edge_m'), ('wgrad', 1, 3, 1, 'steady'), ('wgrad', 3, 2, 1), ('wgrad', 3, 2, 1, 'steady'), ('wgrad', 4, 2, 1), ('wgrad', 4, 2, 1, 'steady'), ('wgrad', 4, 2, 1, 'swapped'), ('wgrad', 5, 2, 0), ('wgrad', 5, 2, 1), ('wgrad', 5, 2, 1, 'steady'), ('wgrad', 5, 3, 1), ('wgrad', 5, 3, 1, 'edge_c'), ('wgrad', 5, 3, 1, 'steady')]),
    ('k5_d96_m1224_H8_td6_B5_wb1', 6, 96, (1, 2, 2, 4), 8, 5, 5, 1,
     [('gn', 1, 1, 1, 0, 0), ('gn', 1, 1, 1, 0, 1), ('gn', 1, 1, 1, 1, 0), ('gn', 1, 1, 1, 1, 1), ('gn', 2, 1, 1, 0, 0), ('gn', 2, 1, 1, 1, 0), ('wgrad', 1, 2, 0, 'part'), ('wgrad', 1, 2, 0, 'steady'), ('wgrad', 5, 0, 0), ('wgrad', 5, 1, 0), ('wgrad', 5, 1, 0, 'part'), ('wgrad', 5, 1, 0, 'steady'), ('wgrad', 5, 2, 0, 'part'), ('wgrad', 5, 2, 0, 'steady'), ('wgrad', 5, 3, 0), ('wgrad', 5, 3, 0, 'edge_c'), ('wgrad', 5, 3, 0, 'part'), ('wgrad', 5, 3, 0, 'steady')]),
    ('k7_d48_m112_H384_td6_B1_wb16', 6, 48, (1, 1, 2), 384, 7, 1, 16,
     [('gn', 4, 1, 1, 0, 0), ('gn', 4, 1, 1, 1, 0), ('gn', 8, 1, 1, 0, 0), ('gn', 8, 1, 1, 1, 0), ('gn', 16, 1, 1, 0, 0), ('gn', 16, 1, 1, 1, 0), ('slabs', '2'), ('slabs', '4'), ('slabs', '8'), ('wgrad', 1, 2, 1), ('wgrad', 1, 2, 1, 'steady'), ('wgrad', 7, 2, 0), ('wgrad', 7, 2, 1), ('wgrad', 7, 2, 1, 'steady'), ('wgrad', 7, 3, 1), ('wgrad', 7, 3, 1, 'edge_c')]),
    ('k7_d48_m14_H32_td6_B3_wb1', 6, 48, (1, 4), 32, 7, 3, 1,
     [('gn', 1, 0, 1, 0, 0), ('gn', 1, 0, 1, 0, 1), ('gn', 1, 0, 1, 1, 0), ('gn', 1, 0, 1, 1, 1), ('gn', 2, 0, 1, 0, 0), ('gn', 2, 0, 1, 1, 0), ('wgrad', 7, 1, 0), ('wgrad', 7, 2, 0, 'part'), ('wgrad', 7, 2, 0, 'steady'), ('wgrad', 7, 3, 0), ('wgrad', 7, 3, 0, 'edge_c'), ('wgrad', 7, 3, 0, 'part'), ('wgrad', 7, 3, 0, 'steady')]),
    ('k3_d64_m1421_H384_td6_B1_wb1', 6, 64, (1, 4, 2, 1), 384, 3, 1, 1,
     [('gn', 0, 1, 0, 0, 0), ('gn', 0, 1, 0, 1, 0), ('gn', 8, 1, 0, 0, 0), ('gn', 8, 1, 0, 1, 0), ('gn', 16, 1, 0, 0, 0), ('gn', 16, 1, 0, 1, 0), ('wgrad', 3, 1, 1), ('wgrad', 3, 1, 1, 'steady'), ('wgrad', 3, 3, 1), ('wgrad', 3, 3, 1, 'edge_c'), ('wgrad', 3, 3, 1, 'steady'), ('wgrad', 4, 1, 1), ('wgrad', 4, 1, 1, 'steady'), ('wgrad', 4, 1, 1, 'swapped')]),
    ('k3_d48_m11_H256_td6_B3', 6, 48, (1, 1), 256, 3, 3, None,
     [('gn', 4, 0, 1, 0, 0), ('gn', 4, 0, 1, 1, 0), ('gn', 8, 0, 1, 0, 0), ('gn', 8, 0, 1, 1, 0), ('slabs', '3'), ('slabs', '6'), ('slabs', 'gt8_mod04')]),
    ('k3_d32_m11_H8_td32_B100', 32, 32, (1, 1), 8, 3, 100, None,
     [('colsums', 'unrolled_tail'), ('resid', 'to_x'), ('slabs', '7'), ('slabs', 'gt8_other')]),
    ('k7_d128_m1421_H8_td6_B13_wb1', 6, 128, (1, 4, 2, 1), 8, 7, 13, 1,
     [('wgrad', 4, 0, 0, 'part'), ('wgrad', 4, 0, 0, 'steady'), ('wgrad', 4, 1, 0, 'part'), ('wgrad', 4, 1, 0, 'steady'), ('wgrad', 7, 0, 0), ('wgrad', 7, 0, 0, 'part'), ('wgrad', 7, 0, 0, 'steady'), ('wgrad', 7, 1, 0, 'part'), ('wgrad', 7, 1, 0, 'steady')]),
    ('k3_d128_m1421_H512_td6_B1_wb1', 6, 128, (1, 4, 2, 1), 512, 3, 1, 1,
     [('gn', 0, 0, 0, 0, 0), ('gn', 0, 0, 0, 1, 0), ('gn', 16, 0, 0, 0, 0), ('gn', 16, 0, 0, 1, 0), ('wgrad', 1, 0, 1), ('wgrad', 1, 0, 1, 'steady'), ('wgrad', 1, 1, 1), ('wgrad', 1, 1, 1, 'steady'), ('wgrad', 3, 0, 1), ('wgrad', 3, 0, 1, 'steady'), ('wgrad', 4, 0, 1), ('wgrad', 4, 0, 1, 'steady'), ('wgrad', 4, 0, 1, 'swapped')]),
    ('k3_d96_m11_H512_td6_B1', 6, 96, (1, 1), 512, 3, 1, None,
     [('gn', 0, 0, 1, 0, 0), ('gn', 0, 0, 1, 1, 0), ('gn', 16, 0, 1, 0, 0), ('gn', 16, 0, 1, 1, 0)]),
    ('k7_d48_m14_H384_td6_B1_wb1', 6, 48, (1, 4), 384, 7, 1, 1,
     [('gn', 0, 1, 1, 0, 0), ('gn', 0, 1, 1, 1, 0), ('wgrad', 7, 1, 1), ('wgrad', 7, 1, 1, 'steady'), ('wgrad', 7, 3, 1, 'steady')]),
    ('k5_d128_m1421_H8_td6_B5_wb1', 6, 128, (1, 4, 2, 1), 8, 5, 5, 1,
     [('wgrad', 5, 0, 0, 'part'), ('wgrad', 5, 0, 0, 'steady')]),
    ('k5_d256_m11_H384_td6_B1_wb1', 6, 256, (1, 1), 384, 5, 1, 1,
     [('wgrad', 5, 0, 1), ('wgrad', 5, 0, 1, 'steady'), ('wgrad', 5, 1, 1), ('wgrad', 5, 1, 1, 'steady')]),
    ('k3_d32_m1_H8_td6_B32_wb1', 6, 32, (1,), 8, 3, 32, 1,
     [('colsums', 'unrolled')]),
    ('k3_d32_m1_H64_td6_B5', 6, 32, (1,), 64, 3, 5, None,
     [('slabs', '5')]),
    ('k7_d256_m11_H384_td6_B1_wb1', 6, 256, (1, 1), 384, 7, 1, 1,
     [('wgrad', 7, 0, 1), ('wgrad', 7, 0, 1, 'steady')]),
]
# registered conv_wgrad kernels not reached in this space (not a claim that they are dead)
NOT_REACHED = [
    # the transposed conv's Z operand is a GroupNorm'd block's gradient and its G operand that block's input: neither ever
    # holds the trajectory's transition_dim columns, the only rows that are not whole aligned float4s (tile 3)
    ('wgrad', 4, 3, 0),
    ('wgrad', 4, 3, 1),
]


# ------------------------------------------------------------------------------------------------ (a)
def _case_steps(case):
    """The step report of a case on an engine without weights (no device call)."""
    _, td, dim, mults, H, ks, B, wb, _ = case
    return census.host_engine(td, dim, mults, H, ks, wb).backward_steps(B)


def _assert_keys(case, rep):
    have = census.step_keys(rep)
    missing = [k for k in case[-1] if tuple(k) not in have]
    assert not missing, f"{case[0]}: the planner no longer takes this case through {missing}; it runs {sorted(have, key=str)}"


def test_matrix_reaches_every_backward_kernel():
    from dynamics_aware_diffusion_amd._engine import wgrad_kernels
    domain = {("wgrad",) + k for k in wgrad_kernels()}
    assert len(domain) == 40
    assert len({c[0] for c in CASES}) == len(CASES)
    reached = set()
    for case in CASES:
        rep = _case_steps(case)
        _assert_keys(case, rep)
        reached |= census.step_keys(rep)
    kernels = {k for k in reached if k[0] == "wgrad" and len(k) == 4}
    listed = {tuple(k) for k in NOT_REACHED}
    assert len(listed) == len(NOT_REACHED)
    both = sorted(kernels & listed)
    assert not both, f"listed as not reached, but the matrix launches them: {both}"
    assert kernels | listed == domain, (sorted(domain - kernels - listed), sorted((kernels | listed) - domain))
    assert len(kernels) == 38
    # every instantiation the matrix launches also runs its double-buffered steady state (>= 2 chunks in a block)
    single = sorted(k for k in kernels if k + ("steady",) not in reached)
    assert not single, f"launched with one chunk per block only: {single}"
    # a part-filled last chunk behind full ones on every tile, either staging path; a partly filled last M and C tile;
    # the transposed conv's swapped roles on every aligned tile, windowed and not
    for tile in range(4):
        assert any(k[0] == "wgrad" and len(k) == 5 and k[2] == tile and k[4] == "part" for k in reached), f"tile {tile}: no part-filled chunk"
    assert any(len(k) == 5 and k[4] == "edge_m" for k in reached) and any(len(k) == 5 and k[4] == "edge_c" for k in reached)
    assert {k[2:4] for k in reached if len(k) == 5 and k[4] == "swapped"} >= {(tile, win) for tile in range(3) for win in (0, 1)}
    # the six forms of the GroupNorm backward, each with and without the d temb store; the wave forms a pair can be short
    # on; a zero-padded horizon and zero-padded groups on the block form, the widest and the narrowest wave form
    # (a key ("gn", nv, 1, ...) says that the form is launched on a padded horizon; it pins the masks of that form only as
    # far as they change a value — the first pass's `live` does not, d A being zero on the padding: module docstring)
    gn = {k[1:] for k in reached if k[0] == "gn"}
    assert {k[0] for k in gn} == set(census.GN_FORMS)
    for nv in census.GN_FORMS:
        assert {k[3] for k in gn if k[0] == nv} == {0, 1}, f"gn form {nv}: d temb written and not"
    for nv in (0, 1, 16):
        assert any(k[0] == nv and k[1] for k in gn) and any(k[0] == nv and k[2] for k in gn), f"gn form {nv}: padded horizon and groups"
    assert any(k[0] == 1 and k[4] for k in gn), "no pair shorter than a wave"
    # the step kinds and the reductions' classes
    for key in [("cols",), ("bias",), ("padcopy",), ("slice_cols",)] + [("resid", k) for k in ("copy", "add", "to_x", "stage")] + \
               [("slabs", str(k)) for k in range(2, 9)] + [("slabs", "gt8_mod04"), ("slabs", "gt8_other")] + \
               [("colsums", k) for k in ("short", "unrolled", "unrolled_tail")]:
        assert key in reached, f"no case runs {key}"


def test_backward_steps_agree_with_backward_plan():
    """The step report's weight-gradient records against the earlier report's, and the refusals of both."""
    from dynamics_aware_diffusion_amd._engine import DadError, HipEngine
    eng = HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=T)
    with pytest.raises(DadError, match="dad_model_set_training"):
        eng.backward_steps(4)
    eng = census.host_engine(6, 32, (1, 2, 4), 24, 5)
    with pytest.raises(DadError):
        eng.backward_steps(0)
    for B in (1, 4, 250):
        plan, rep = eng.backward_plan(B), eng.backward_steps(B)
        wg = [q for q in rep["steps"] if q["kind"] == "wgrad"]
        assert len(wg) == plan["wgrads"] == 35 and rep["batch"] == B
        for a, b in zip(plan["launches"], wg):
            assert all(a[f] == b[f] for f in a), (a, b)
        assert rep["padcopy"] and (rep["horizon"], rep["real_horizon"]) == (32, 24) and rep["dx"]
        assert rep["colsums"][0] == 1 and rep["colsums"][1] == 3 * sum(q["kind"] == "gn" for q in rep["steps"]) + \
            sum(q["kind"] == "bias" for q in rep["steps"])
        assert sum(q["kind"] == "dgrad" for q in rep["steps"]) == sum(plan["dgrad"].values())


# ------------------------------------------------------------------------------------------------ (b)
def _inputs(name, B, H, td):
    from dynamics_aware_diffusion_amd.utils import synth
    x0 = np.clip(synth.normal_like(29, f"bpath.x.{name}", (B, H, td)) * 0.5, -1, 1).astype(np.float32)
    t = np.array([(3 * i + 1) % T for i in range(B)], dtype=np.int64)
    t[-1] = T - 1
    noise = synth.normal_like(29, f"bpath.n.{name}", (B, H, td))
    return x0, t, noise


@functools.lru_cache(maxsize=None)
def _reference(name, td, dim, mults, H, ks, B, seed=SEED):
    """Weights, inputs and the float64 oracle of a case with the fp32 oracle's own distance from it, computed once;
    nobody writes into it.  (tests/backward_census.py --check-oracle asks too.)"""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    state = synth.synth_unet_state(td, dim, mults, seed=seed, affine_jitter=0.3, kernel_size=ks)
    x0, t, noise = _inputs(name, B, H, td)
    w = as_torch(state)
    sched = orc.schedule_buffers("cosine", T)
    x0t, tt, nz = torch.from_numpy(x0), torch.from_numpy(t), torch.from_numpy(noise)
    w64 = orc.cast_weights(w, torch.float64)
    s64 = {k: v.double() for k, v in sched.items()}
    l64, g64, dx64 = orc.training_gradients(w64, s64, x0t.double(), tt, nz.double())
    _, _, out64 = orc.training_loss(w64, s64, x0t.double(), tt, nz.double())
    _, g32, dx32 = orc.training_gradients(w, sched, x0t, tt, nz)
    _, _, out32 = orc.training_loss(w, sched, x0t, tt, nz)
    scales = grad_scales(g64)
    orc_errs = {k: max_abs(g32[k].numpy(), g64[k].numpy()) / scales[k] for k in g64}
    orc_errs["d x_t"] = max_abs(dx32.numpy(), dx64.numpy()) / float(dx64.abs().max())
    return {"state": state, "inputs": (x0, t, noise), "l64": l64, "g64": g64, "dx64": dx64, "out64": out64, "scales": scales,
            "orc_errs": orc_errs, "o_out": max_abs(out32.numpy(), out64.numpy())}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_backward_case_vs_float64(case, dev):
    from tests.test_hip_long_horizon import _diffusion
    from tests.test_hip_train_batch import _train_step
    name, td, dim, mults, H, ks, B, wb, keys = case
    ref = _reference(name, td, dim, mults, H, ks, B)
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, ref["state"], dev, ks=ks)
    eng = diff.model.engine(H, dev, training=True)
    x0, t, noise = ref["inputs"]
    try:
        if wb is not None:
            eng.debug_set_option("wgrad_blocks", wb)
        _assert_keys(case, eng.backward_steps(B))
        loss, out, dx, grads = _train_step(diff, x0, t, noise, dev)
        loss2, out2, dx2, grads2 = _train_step(diff, x0, t, noise, dev)
        assert diff.model._engine is eng, "the engine was rebuilt: the steps asserted above are not the ones that ran"
    finally:
        eng.debug_set_option("wgrad_blocks", 256)
    l64, g64, dx64, out64, scales, orc_errs, o_out = (ref[k] for k in ("l64", "g64", "dx64", "out64", "scales", "orc_errs", "o_out"))
    assert set(grads) == set(g64)
    errs = {k: max_abs(grads[k], g64[k].numpy()) / scales[k] for k in grads}
    errs["d x_t"] = max_abs(dx, dx64.numpy()) / float(dx64.abs().max())
    worst, oworst = max(errs, key=errs.get), max(orc_errs, key=orc_errs.get)
    e_out = max_abs(out, out64.numpy())
    e_loss = abs(loss - float(l64)) / max(1.0, abs(float(l64)))
    print(f"\n{name}: gradients vs float64, x max|g|: engine {errs[worst]:.2e} ({worst}), d x_t {errs['d x_t']:.2e}; "
          f"fp32 oracle {orc_errs[oworst]:.2e} ({oworst}), d x_t {orc_errs['d x_t']:.2e}\n"
          f"  training-forward output vs float64: engine {e_out:.2e}, fp32 oracle {o_out:.2e}; loss: engine {e_loss:.1e} relative")
    # the condition a case is admitted on: the fp32 oracle itself within REL / 2 of float64 on every tensor, or the gate
    # could not tell a wrong kernel from fp32
    far = {k: f"{e:.2e}" for k, e in orc_errs.items() if not e <= ADMIT}
    assert not far, f"{name}: the fp32 oracle is farther than {ADMIT} x max|g| from float64: {far}"
    for k in grads:
        assert np.isfinite(grads[k]).all(), k
    bad = {k: f"{e:.2e}" for k, e in errs.items() if not e <= REL}
    assert not bad, f"{name}: gradients farther than {REL} x max|g| from float64: {bad}"
    assert e_out <= TOL_STEP, f"{name}: training-forward output {e_out:.2e} from the float64 forward"
    assert e_loss <= LOSS_REL, f"{name}: loss {loss} vs {float(l64)}"
    assert loss == loss2 and np.array_equal(out, out2) and np.array_equal(dx, dx2), f"{name}: a second call gives other bits"
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), f"{name}: {k} differs between two calls"
