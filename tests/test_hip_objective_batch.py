"""The fused training objective (``GaussianDiffusion.fused_objective``; csrc/train_objective.hpp) at the batch sizes
training runs and at the edges of its time chain, where tests/test_hip_objective.py (batches <= 9, one case at 250)
does not reach:

  time_gemm_kernel   eight modes; per mode one K chunk (three idle waves), several chunks per wave, chunk counts the four
                     waves do not share evenly, a K tail inside a chunk (K % 32), ragged M and N, grids of several tiles
  TG_BWD_DACT        1 / >= 3 K slices, a last slice shorter than the others, slices of 2 and more chunks per wave;
                     time_dtemb_kernel adds the slabs
  bias gradients     the eight row groups with unequal trips behind several full ones (B = 250), one row (B = 1)
  loss reduction     1 partial, 320 (the final kernel's stride loop takes a second trip), the cap of 1024 with more
                     than four elements per thread (n > 2^20)
  time_dim           20 / 40 / 72 / 100 / 264 / 8 against dim 32: ragged in M, N and K

(a) test_matrix_reaches_every_time_chain_path (no device): every case asks Engine.objective_plan
    (dad_debug_objective_plan: the list of launches the two entry points replay) for the property it exists for; the
    matrix as a whole reaches every (mode, property) pair above that the mode can reach at all (EXEMPT lists the rest
    with the reason).
(b) test_fused_objective_vs_float64: every parameter gradient, the loss, x_t (bit-equal to q_sample) and the kept
    output against the oracle in float64; a second call bit for bit equal; the unfused path on the same draws.
(c) test_l1_at_exact_ties: L1 with out == 0 exactly and exact zeros in the noise: sign(0) = 0.
(d) test_rows_of_a_large_fused_batch_match_a_small_one: rows 0..8 of a batch-250 forward against the batch-9 forward.

The matrix is the eleven LARGE shapes of tests/test_hip_train_batch.py (same draws, same float64 oracle: computed once
per run by its _large_oracle) plus the cases of EXTRA.  Beyond the cases this module was first planned with, EXTRA holds
td100_B512 (no named case has a short last K slice — the planner gives PointMaze at batch 250 seven full slices of
512, not eight — nor a partial count between 256 and 1024), td264_B512 (none has kslices == 1: that needs more than
128 output tiles) and td8_B5 (TG_FWD_TEMB with one K chunk needs time_dim <= 8).  `cap` is the shape as named
(td 17, dim 32, mults (1, 2), H 128, B 512: n = 1 114 112); the engine accepts it.

Gates (none new): gradients |g - g_f64| <= 2e-5 max|g_f64| per tensor (REL; scales by tests/util.grad_scales), loss
2e-6 relative, kept output <= TOL_STEP (5e-6) from the float64 forward, x_t bit-equal.  L1 appears only in (c) and in
the small reference fixtures: at training batches a sign flip of one element whose |out - target| is below fp32
rounding moves a gradient by 2 w / n, which is the objective's conditioning and not the kernel's.

Measured on an MI355X (`-s` prints every case).  (b), 21 cases: fused gradients 3.7e-7 .. 3.0e-6 max|g| from float64
(worst: downs.0.0.blocks.0.block.1.weight of td72, where the fp32 oracle is at 2.9e-6 and the unfused path at 2.2e-6),
the time-chain tensors alone <= 1.5e-6 (time_mlp.1.weight of B33_same_t); the fp32 oracle 1.4e-6 .. 5.7e-6, the
unfused path 5.0e-7 .. 2.2e-6, fused against unfused <= 3.2e-6 (train_py_defaults_B128); kept outputs 6.5e-7 ..
1.6e-6 (fp32 oracle 9.8e-7 .. 2.1e-6); loss <= 9.8e-8 relative; x_t bit-equal and the second call bit-identical in
every case.  (c) loss 1.8e-8 relative, final_conv.1.bias.grad 1.1e-7, final_conv.1.weight.grad 2.4e-7 max|g|, all other
gradients exactly 0.  (d) outputs 1.25e-6 apart (1.04e-6 / 7.6e-7 from float64).  No case had to be exchanged.

Four deliberate one-line arithmetic errors, each run once against tests/test_hip_objective.py (20 tests) and this
module (23 GPU tests).  The first three were ALREADY caught by tests/test_hip_objective.py; only the fourth was not:
  1. time_gemm_kernel's epilogue without the fourth wave's partial: the old module failed 17 of 20 (every test that
     compares values: K = 4 time_dim = 128 is four chunks on the smallest net), this module all 23.
  2. time_dtemb_kernel adding ks - 1 slabs: the old module failed 15 of 20 (every net has >= 3 slices; the five that
     hold no gradient to a reference passed), this
     module 20 of 23: all of (b) but td264_B512 (one slice: nothing to leave out); (c) (all upstream gradients are 0
     there) and (d) (forward only) passed.
  3. the bias-gradient loop stepping by 16: the old module failed only its two cases with a batch above 8
     (grads_pointmaze_B9, test_fused_pointmaze_batch_250_vs_float64) and passed the other 18; this module failed 19 of
     (b): all but B1 and td8_B5 (batches of 8 and less never reach a second trip); (c) and (d) passed as under 2.
  4. objective_loss_final_kernel reading partial[threadIdx.x] only: the old module passed all 20 (at most 47
     partials); here td100_B512 (320 partials) and cap (1024) failed, everything else passed.
"""
import functools

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_hip_objective import _step, fused
from tests.test_hip_parity import TOL_STEP, dev  # noqa: F401  (dev: fixture)
from tests.test_hip_train_batch import LARGE, T, _host_engine, _inputs, _large_oracle, _set_knob
from tests.util import as_torch, grad_scales, max_abs

REL = 2e-5
MODES = ("FWD_H1", "FWD_TEMB", "FWD_ROWS", "BWD_DWK", "BWD_DACT", "BWD_DW3", "BWD_DH1", "BWD_DW1")


# ------------------------------------------------------------------------------------------------ the matrix
def _l(plan, mode):
    return next(q for q in plan["launches"] if q["mode"] == mode)


def _most(q):
    return max(q["chunks"], q["last_chunks"])


# what a launch can show: name -> predicate on its record
PROPERTIES = {
    "one K chunk (three idle waves)": lambda q: q["chunks"] == 1 or q["last_chunks"] == 1,
    "two or more chunks on a wave": lambda q: _most(q) >= 5,
    "chunks the four waves do not share evenly": lambda q: q["chunks"] % 4 != 0 or q["last_chunks"] % 4 != 0,
    "a K tail inside a chunk": lambda q: q["ktail"] != 0,
    "ragged M": lambda q: q["M"] % 32 != 0,
    "ragged N": lambda q: q["N"] % 32 != 0,
    "several tiles in x": lambda q: q["grid"][0] > 1,
    "several tiles in y": lambda q: q["grid"][1] > 1,
}
# (mode, property) pairs no architecture reaches, with the reason
_W128 = "temb_width is 4 x the sum of the (padded) channel counts, each a multiple of 32: a multiple of 128"
_DIM32 = "the engine pads dim to a multiple of 32 (a dim of 40 runs as 64)"
EXEMPT = {
    ("FWD_H1", "a K tail inside a chunk"): "K = dim: " + _DIM32,
    ("BWD_DW1", "ragged N"): "N = dim: " + _DIM32,
    ("FWD_ROWS", "ragged N"): "N = temb_width: " + _W128,
    ("BWD_DWK", "ragged M"): "M = temb_width: " + _W128,
    ("BWD_DACT", "one K chunk (three idle waves)"): "K = temb_width in slices of whole 128s: " + _W128,
    ("BWD_DACT", "chunks the four waves do not share evenly"): "K = temb_width in slices of whole 128s: " + _W128,
    ("BWD_DACT", "a K tail inside a chunk"): "K = temb_width: " + _W128,
}


def _dact(pred):
    return lambda p: pred(_l(p, "BWD_DACT"), p)


# the fused properties of the LARGE shapes (tests/test_hip_train_batch.py), by name
LARGE_PROPS = {
    "pointmaze_B256": [("d act in 7 full slices of 512 columns: 16 chunks, 4 per wave", _dact(lambda q, p: p["kslices"] == 7 and q["chunks"] == q["last_chunks"] == 16)),
                       ("every launch on whole tiles and whole chunks", lambda p: all(q["M"] % 32 == q["N"] % 32 == q["ktail"] == 0 for q in p["launches"] if q["mode"] != "DTEMB"))],
    "pointmaze_B250": [("batch as K: 8 chunks with a tail of 26, two per wave", lambda p: all(_l(p, m)["chunks"] == 8 and _l(p, m)["ktail"] == 26 for m in ("BWD_DWK", "BWD_DW3", "BWD_DW1"))),
                       ("bias-gradient row groups with unequal trips behind 31 full ones", lambda p: _l(p, "BWD_DWK")["K"] == 250),
                       ("ragged M in all five launches with the batch as M", lambda p: sum(q["M"] == 250 for q in p["launches"] if q["mode"] != "DTEMB") == 5),
                       ("47 partial sums", lambda p: p["loss_blocks"] == 47)],
    "train_py_defaults_B128": [("four levels: 16 residual blocks, 15 slices of one chunk per wave", lambda p: p["blocks"] == 16 and p["kslices"] == 15 and _l(p, "BWD_DACT")["chunks"] == 4)],
    "halfcheetah_B32": [("HalfCheetah widths: 26 slices of 512 over temb_width 13312", lambda p: p["kslices"] == 26 and p["kslice"] == 512 and p["temb_width"] == 13312),
                        ("K = dim = time_dim = 256: 8 chunks; K = 4 time_dim: 32", lambda p: _l(p, "FWD_H1")["chunks"] == _l(p, "FWD_ROWS")["chunks"] == _l(p, "BWD_DH1")["chunks"] == 8 and _l(p, "FWD_TEMB")["chunks"] == 32),
                        ("the batch as one K chunk", lambda p: _l(p, "BWD_DWK")["chunks"] == 1 and _l(p, "BWD_DWK")["grid"] == (416, 8, 1))],
    "c2048_B96": [("two levels: 8 residual blocks; slices of 1024 columns, 8 chunks per wave", lambda p: p["blocks"] == 8 and p["kslice"] == 1024 and _l(p, "BWD_DACT")["chunks"] == 32),
                  ("the batch as 3 chunks: one idle wave", lambda p: _l(p, "BWD_DW3")["chunks"] == 3)],
    "tiny_B512": [("the batch as 16 chunks", lambda p: _l(p, "BWD_DW1")["chunks"] == 16), ("96 partial sums", lambda p: p["loss_blocks"] == 96)],
    "H256_B96": [("144 partial sums over 147456 elements", lambda p: p["loss_blocks"] == 144 and p["n"] == 147456)],
    "H256_B24_wb16": [("a batch below one tile: K = 24 inside one chunk", lambda p: _l(p, "BWD_DWK")["ktail"] == 24 and _l(p, "BWD_DWK")["chunks"] == 1)],
    "k3_B512": [("dim = time_dim = 64: two chunks, two idle waves; slices of two chunks per wave", lambda p: _l(p, "FWD_H1")["chunks"] == 2 and _l(p, "BWD_DACT")["chunks"] == 8)],
    "k7_B250_wb16": [("two levels at batch 250: 5 slices", lambda p: p["blocks"] == 8 and p["kslices"] == 5 and _l(p, "BWD_DW3")["ktail"] == 26)],
    "d96_H24_B128": [("padded net: dim runs as 128, time_dim stays 96 (3 chunks), temb_width 3584 padded", lambda p: _l(p, "FWD_H1")["K"] == 128 and _l(p, "FWD_ROWS")["K"] == 96 and p["temb_width"] == 3584),
                     ("the mean counts the real elements only", lambda p: p["n"] == 128 * 24 * 6),
                     ("14 slices", lambda p: p["kslices"] == 14)],
}

# (id, td, dim, mults, horizon, batch, time_dim or None, what is special about the draws, why, [(property, predicate)])
EXTRA = [
    ("td20", 6, 32, (1, 2, 4), 32, 33, 20, None, "time_dim 20: ragged M / N / K, K tails of 16 and 20 inside a chunk", [
        ("K = 80 in three chunks with a tail of 16", lambda p: _l(p, "FWD_TEMB")["chunks"] == 3 and _l(p, "FWD_TEMB")["ktail"] == 16),
        ("K = time_dim = 20 in one part-filled chunk", lambda p: _l(p, "FWD_ROWS")["ktail"] == _l(p, "BWD_DH1")["ktail"] == 20),
        ("ragged N in six modes", lambda p: sum(q["N"] % 32 != 0 for q in p["launches"] if q["mode"] != "DTEMB") == 6),
        ("batch 33: one row in the second tile and the second chunk", lambda p: _l(p, "BWD_DWK")["chunks"] == 2 and _l(p, "BWD_DWK")["ktail"] == 1),
    ]),
    ("td40", 6, 32, (1, 2, 4), 32, 96, 40, None, "time_dim 40: K tail of 8, five chunks over four waves", [
        ("K = 160: five chunks, wave 0 takes two", lambda p: _l(p, "FWD_TEMB")["chunks"] == 5),
        ("K = 40: a tail of 8 in the second chunk", lambda p: _l(p, "FWD_ROWS")["chunks"] == 2 and _l(p, "FWD_ROWS")["ktail"] == 8),
    ]),
    ("td72", 6, 32, (1, 2, 4), 32, 31, 72, None, "time_dim 72 at a batch one short of a tile", [
        ("K = 288: nine chunks, wave 0 takes three", lambda p: _l(p, "FWD_TEMB")["chunks"] == 9),
        ("K = 72: three chunks, the last of 8", lambda p: _l(p, "BWD_DH1")["chunks"] == 3 and _l(p, "BWD_DH1")["ktail"] == 8),
        ("batch 31 as K: one part-filled chunk", lambda p: _l(p, "BWD_DW3")["ktail"] == 31 and _l(p, "BWD_DW3")["chunks"] == 1),
    ]),
    ("B1", 6, 32, (1, 2, 4), 32, 1, None, None, "batch 1", [
        ("one row, one partial sum", lambda p: p["loss_blocks"] == 1 and _l(p, "BWD_DWK")["K"] == 1 and _l(p, "FWD_H1")["M"] == 1),
    ]),
    ("B33_same_t", 6, 32, (1, 2, 4), 32, 33, None, "same_t", "every row at the same timestep: identical rows of the time chain", [
        ("batch 33", lambda p: _l(p, "FWD_H1")["grid"][0] == 2),
    ]),
    ("pointmaze_B250_w", 6, 128, (1, 2, 4), 32, 250, None, "weighted", "the weighted mean at a training batch", [
        ("47 partial sums", lambda p: p["loss_blocks"] == 47),
    ]),
    ("cap", 17, 32, (1, 2), 128, 512, None, None, "n = 1 114 112 > 2^20: 1024 partial sums, more than four elements per thread", [
        ("the cap of 1024 partial sums holds", lambda p: p["loss_blocks"] == 1024 and p["n"] == 1114112 > 4 * 256 * 1024),
        ("three slices", lambda p: p["kslices"] == 3),
    ]),
    ("td100_B512", 20, 32, (1, 2, 4), 32, 512, 100, None, "a short last K slice; 320 partial sums", [
        ("four slices of 256 columns over 896: the last holds 128", _dact(lambda q, p: p["kslices"] == 4 and q["chunks"] == 8 and q["last_chunks"] == 4)),
        ("320 partial sums: the final kernel's loop takes a second trip", lambda p: p["loss_blocks"] == 320),
        ("K = 400: 13 chunks with a tail of 16; K = 100: a tail of 4", lambda p: _l(p, "FWD_TEMB")["chunks"] == 13 and _l(p, "FWD_ROWS")["ktail"] == 4),
    ]),
    ("td264_B512", 6, 32, (1, 2, 4), 8, 512, 264, None, "more than 128 output tiles: d act in one slice", [
        ("one slice of 896 columns: 28 chunks, 7 per wave", _dact(lambda q, p: p["kslices"] == 1 and q["chunks"] == 28 and q["grid"] == (16, 9, 1))),
        ("K = 1056: 33 chunks, wave 0 takes nine", lambda p: _l(p, "FWD_TEMB")["chunks"] == 33),
    ]),
    ("td8_B5", 6, 32, (1, 2), 32, 5, 8, None, "time_dim 8: every K of the chain inside one chunk", [
        ("K = 4 time_dim = 32: one chunk", lambda p: _l(p, "FWD_TEMB")["chunks"] == 1),
        ("K = 8 and K = 5", lambda p: _l(p, "BWD_DH1")["ktail"] == 8 and _l(p, "BWD_DW1")["ktail"] == 5),
    ]),
]

# every case in one form: (id, td, dim, mults, H, B, kernel_size, wgrad_blocks, time_dim, draws, why, properties)
MATRIX = [(n, td, dim, mults, H, B, ks, wb, None, None, why, LARGE_PROPS[n]) for n, td, dim, mults, H, B, ks, wb, why, _ in LARGE] + \
         [(n, td, dim, mults, H, B, 5, None, tdm, draws, why, props) for n, td, dim, mults, H, B, tdm, draws, why, props in EXTRA]


def _assert_objective_path(label, plan, props):
    for text, pred in props:
        assert pred(plan), f"{label}: the planner no longer gives '{text}': " \
                           f"{ {k: v for k, v in plan.items() if k != 'launches'} } {plan['launches']}"
    return "; ".join(text for text, _ in props)


def test_matrix_reaches_every_time_chain_path():
    """No device needed.  Each case's own properties hold, and together the cases reach every path of the time chain
    and of the loss reduction this module exists for; a retuned planner that lets a case fall off its path fails here."""
    assert len(LARGE) == 11 and set(LARGE_PROPS) == {c[0] for c in LARGE} and len(MATRIX) == 11 + len(EXTRA)
    plans = []
    for name, td, dim, mults, H, B, ks, wb, tdm, _, _, props in MATRIX:
        eng = _host_engine(td, dim, mults, H, ks, tdm)
        if wb is not None:
            _set_knob(eng, "wgrad_blocks", wb)
        plan = eng.objective_plan(B)
        _assert_objective_path(name, plan, props)
        assert [q["mode"] for q in plan["launches"]] == ["FWD_H1", "FWD_TEMB", "FWD_ROWS", "BWD_DWK", "BWD_DACT", "DTEMB", "BWD_DW3", "BWD_DH1", "BWD_DW1"]
        plans.append((name, B, plan))
    # every mode x every property, or an exemption with its reason: nothing silently absent, no exemption that is reached
    for mode in MODES:
        for text, pred in PROPERTIES.items():
            reached = [name for name, _, plan in plans if pred(_l(plan, mode))]
            if (mode, text) in EXEMPT:
                assert not reached, f"{mode}: '{text}' is exempt ({EXEMPT[(mode, text)]}) but {reached} reach it"
            else:
                assert reached, f"no case runs TG_{mode} with {text}"
    assert all(m in MODES and t in PROPERTIES for m, t in EXEMPT)
    # what the exemptions rest on
    assert all(plan["temb_width"] % 128 == 0 and _l(plan, "FWD_H1")["K"] % 32 == 0 for _, _, plan in plans)
    assert _l(_host_engine(6, 40, (1, 2), 32, 5).objective_plan(5), "FWD_H1")["K"] == 64
    # d act = d rows . W: one slice, three and more, a last slice shorter than the others, a slice of >= 2 chunks per wave
    dact = [(plan["kslices"], _l(plan, "BWD_DACT")) for _, _, plan in plans]
    assert any(ks == 1 for ks, _ in dact) and any(ks >= 3 for ks, _ in dact)
    assert any(ks > 1 and q["last_chunks"] < q["chunks"] for ks, q in dact)
    assert any(ks > 1 and q["chunks"] >= 8 for ks, q in dact) and any(q["kslice"] > 128 for _, q in dact)
    assert all(q["kslice"] % 128 == 0 and (ks - 1) * q["kslice"] < q["K"] <= ks * q["kslice"] for ks, q in dact)
    # the loss reduction: one partial, a second trip of the final kernel's stride-256 loop below the cap, the cap with
    # more than four elements per thread
    blocks = [(plan["loss_blocks"], plan["n"]) for _, _, plan in plans]
    assert any(b == 1 for b, _ in blocks) and any(256 < b < 1024 for b, _ in blocks)
    assert any(b == 1024 and n > 1 << 20 for b, n in blocks) and all(b == min(1024, -(-n // 1024)) for b, n in blocks)
    # bias gradients: eight row groups, unequal trips behind several full ones; one row
    assert any(B % 8 != 0 and B >= 57 for _, B, _ in plans) and any(B == 1 for _, B, _ in plans)
    assert {31, 33} <= {B for _, B, _ in plans}
    # 4-level and 2-level nets
    assert {8, 12, 16} <= {plan["blocks"] for _, _, plan in plans}


# ------------------------------------------------------------------------------------------------ (b)
def _diffusion(td, dim, mults, H, state, devc, ks=5, time_dim=None, **kw):
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    unet = TemporalUnet(td, dim=dim, dim_mults=mults, time_dim=time_dim, kernel_size=ks)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return GaussianDiffusion(unet, H, td - 1, 1, n_timesteps=T, **kw).to(devc)


@functools.lru_cache(maxsize=None)
def _extra_oracle(name):
    """As _large_oracle of tests/test_hip_train_batch.py for a case of EXTRA (with its weights, where it has them)."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    _, td, dim, mults, H, B, tdm, draws, _, _ = next(c for c in EXTRA if c[0] == name)
    state = synth.synth_unet_state(td, dim, mults, seed=43, affine_jitter=0.3, time_dim=tdm)
    x0, t, noise = _inputs(name, B, H, td)
    if draws == "same_t":
        t[:] = 7
    wts = (1.0 + synth.uniform(20, f"obatch.w.{name}", (1, H, td), 0.5)).astype(np.float32) if draws == "weighted" else None
    w = as_torch(state)
    sched = orc.schedule_buffers("cosine", T)
    x0t, tt, nz = torch.from_numpy(x0), torch.from_numpy(t), torch.from_numpy(noise)
    wt = None if wts is None else torch.from_numpy(wts)
    w64 = orc.cast_weights(w, torch.float64)
    s64 = {k: v.double() for k, v in sched.items()}
    l64, g64, _ = orc.training_gradients(w64, s64, x0t.double(), tt, nz.double(), "l2", True, None if wt is None else wt.double())
    _, _, out64 = orc.training_loss(w64, s64, x0t.double(), tt, nz.double())
    _, g32, _ = orc.training_gradients(w, sched, x0t, tt, nz, "l2", True, wt)
    _, _, out32 = orc.training_loss(w, sched, x0t, tt, nz)
    scales = grad_scales(g64)
    return {"state": state, "inputs": (x0, t, noise), "weights": wts, "l64": l64, "g64": g64, "out64": out64, "scales": scales,
            "orc_errs": {k: max_abs(g32[k].numpy(), g64[k].numpy()) / scales[k] for k in g64}, "o_out": max_abs(out32.numpy(), out64.numpy())}


@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=lambda c: c[0])
def test_fused_objective_vs_float64(case, dev):
    name, td, dim, mults, H, B, ks, wb, tdm, draws, why, props = case
    ref = _large_oracle(name) if name in LARGE_PROPS else _extra_oracle(name)
    diff = _diffusion(td, dim, mults, H, ref["state"], dev, ks=ks, time_dim=tdm)
    diff._engine(dev)                      # (binds the schedule and the diffusion's options to the model)
    eng = diff.model.engine(H, dev, training=True)
    if wb is not None:
        eng.debug_set_option("wgrad_blocks", wb)
    path = _assert_objective_path(name, eng.objective_plan(B), props)
    x0, t, noise = ref["inputs"]
    wts = ref.get("weights")
    with fused(diff):
        loss, grads = _step(diff, x0, t, noise, wts, dev)
        loss2, grads2 = _step(diff, x0, t, noise, wts, dev)
    assert type(loss.grad_fn).__name__ == "_ObjectiveFunctionBackward"
    l_off, g_off = _step(diff, x0, t, noise, wts, dev)                  # the unfused path on the same draws
    assert type(l_off.grad_fn).__name__ != "_ObjectiveFunctionBackward"
    assert diff.model._engine is eng, "the engine was rebuilt: the plan asserted above is not the one that ran"
    # x_t and the output the fused forward keeps
    x0t, nz = torch.from_numpy(x0).to(dev), torch.from_numpy(noise).to(dev)
    tt = torch.from_numpy(t).to(dev)
    eng.bind_train_schedule(diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod)
    wfull = None if wts is None else torch.from_numpy(wts).to(dev).expand(x0t.shape).contiguous()
    loss3, saved = eng.objective_forward(x0t, tt.to(torch.int32), nz, wfull, 2)
    xt, out = eng.objective_saved_views(saved, B)
    want_xt = diff.q_sample(x0t, tt, nz)
    torch.cuda.synchronize()
    assert torch.equal(xt, want_xt), f"{name}: x_t differs from q_sample by {float((xt - want_xt).abs().max()):.3e}"
    assert float(loss3) == float(loss)

    l64, g64, out64, scales, orc_errs = (ref[k] for k in ("l64", "g64", "out64", "scales", "orc_errs"))
    assert set(grads) == set(g64) == set(g_off)
    assert any(k.startswith("time_mlp.") for k in grads) and sum(".time_mlp.1." in k for k in grads) == 2 * eng.objective_plan(B)["blocks"]
    errs = {k: max_abs(grads[k], g64[k].numpy()) / scales[k] for k in grads}
    off_errs = {k: max_abs(g_off[k], g64[k].numpy()) / scales[k] for k in grads}
    route = {k: max_abs(grads[k], g_off[k]) / scales[k] for k in grads}
    worst, oworst, fworst, rworst = (max(d, key=d.get) for d in (errs, orc_errs, off_errs, route))
    tworst = max((k for k in errs if "time_mlp." in k), key=errs.get)
    e_out = max_abs(out.cpu().numpy(), out64.numpy())
    e_loss = abs(float(loss) - float(l64)) / max(1.0, abs(float(l64)))
    print(f"\n{name} ({why})\n  path: {path}\n  gradients vs float64, x max|g|: fused {errs[worst]:.2e} ({worst}; there: fp32 oracle {orc_errs[worst]:.2e}, "
          f"unfused {off_errs[worst]:.2e}), worst time-chain tensor {errs[tworst]:.2e} ({tworst}); fp32 oracle {orc_errs[oworst]:.2e} ({oworst}); "
          f"unfused {off_errs[fworst]:.2e} ({fworst}); fused vs unfused {route[rworst]:.2e} ({rworst})\n"
          f"  kept output vs float64: fused {e_out:.2e}, fp32 oracle {ref['o_out']:.2e}; loss: fused {e_loss:.1e} relative")
    for k in grads:
        assert np.isfinite(grads[k]).all(), k
    bad = {k: f"{e:.2e} (fp32 oracle {orc_errs[k]:.2e}, unfused {off_errs[k]:.2e})" for k, e in errs.items() if not e <= REL}
    assert not bad, f"{name}: fused gradients farther than {REL} x max|g| from float64: {bad}"
    assert e_loss <= 2e-6, f"{name}: loss {float(loss)} vs {float(l64)}"
    assert e_out <= TOL_STEP, f"{name}: kept output {e_out:.2e} from the float64 forward"
    bad = {k: f"{e:.2e}" for k, e in route.items() if not e <= REL}
    assert not bad, f"{name}: fused and unfused gradients farther apart than {REL} x max|g|: {bad}"
    assert abs(float(loss) - float(l_off)) <= 2e-6 * max(1.0, abs(float(l_off)))
    # fixed-order reductions: a second call gives the same bits
    assert float(loss) == float(loss2)
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), f"{name}: {k} differs between two calls"


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.gpu
def test_l1_at_exact_ties(dev):
    """The tiny net with final_conv.1 zeroed: out == 0 exactly, so out - noise is an exact tie wherever the noise is 0.
    loss = mean(w |noise|); d loss / d out = -sign(noise) w / n with 0 at the ties (torch's sign(0) = 0);
    final_conv.1.bias.grad is its column sum; final_conv.1.weight.grad that tensor against the last activation (held to
    the float64 oracle); every other gradient is exactly 0."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    net, B, H = "tiny", 33, cases.H
    _, _, td, dim, mults = cases.net_dims(net)
    state = {k: v.copy() for k, v in cases.net_weights(net).items()}
    state["final_conv.1.weight"][:] = 0.0
    state["final_conv.1.bias"][:] = 0.0
    diff = _diffusion(td, dim, mults, H, state, dev, loss_type="l1", predict_epsilon=True)
    x0, t, noise = (a.copy() for a in _inputs("l1_ties", B, H, td))
    n = noise.size
    noise.reshape(-1)[3::8] = 0.0                                                  # a fixed eighth: exact ties
    wts = (1.0 + synth.uniform(20, "obatch.w.l1_ties", (B, H, td), 0.5)).astype(np.float32)
    wts.reshape(-1)[::5] = 0.0                                                     # some weights exactly 0
    assert np.count_nonzero(noise == 0) == n // 8 and np.count_nonzero((noise == 0) & (wts != 0)) > 100
    with fused(diff):
        loss, grads = _step(diff, x0, t, noise, wts, dev)
    assert type(loss.grad_fn).__name__ == "_ObjectiveFunctionBackward"
    n64, w64 = noise.astype(np.float64), wts.astype(np.float64)
    want_loss = float((w64 * np.abs(n64)).mean())
    d_out = -np.sign(n64) * w64 / n
    assert np.count_nonzero(d_out == 0) >= n // 8
    e_loss = abs(float(loss) - want_loss) / max(1.0, want_loss)
    want_b = d_out.sum(axis=(0, 1))
    e_b = max_abs(grads["final_conv.1.bias"], want_b) / float(np.abs(want_b).max())
    # the one other non-zero gradient, against the oracle's autograd in float64 (same sign convention)
    w64t = orc.cast_weights(as_torch(state), torch.float64)
    s64 = {k: v.double() for k, v in orc.schedule_buffers("cosine", T).items()}
    l64, g64, _ = orc.training_gradients(w64t, s64, torch.from_numpy(x0).double(), torch.from_numpy(t), torch.from_numpy(noise).double(),
                                         "l1", True, torch.from_numpy(wts).double())
    assert abs(float(l64) - want_loss) <= 1e-12 and max_abs(g64["final_conv.1.bias"].numpy(), want_b) <= 1e-12
    kw = "final_conv.1.weight"
    e_w = max_abs(grads[kw], g64[kw].numpy()) / float(g64[kw].abs().max())
    print(f"\nL1 at exact ties: loss {e_loss:.1e} relative, final_conv.1.bias.grad {e_b:.2e} x max|g|, final_conv.1.weight.grad {e_w:.2e} x max|g|")
    assert e_loss <= 2e-6
    assert e_b <= REL and e_w <= REL
    for k, g in grads.items():
        if not k.startswith("final_conv.1."):
            assert np.array_equal(g, np.zeros_like(g)), f"{k}: a gradient upstream of the zeroed conv is not exactly 0 (max {np.abs(g).max():.3e})"


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.gpu
def test_rows_of_a_large_fused_batch_match_a_small_one(dev):
    """objective_forward of pointmaze_B250 and of its rows 0..8 as a batch of 9: x_t of the nine rows bit-equal, the
    kept outputs within TOL_STEP of each other and of the float64 forward.  The time projections have no accessor of
    their own (dad_debug_objective_offsets names x_t and the output only), so they are compared through the output
    they enter in every residual block."""
    name, td, dim, mults, H, B, ks = LARGE[1][:7]
    assert name == "pointmaze_B250"
    ref = _large_oracle(name)
    diff = _diffusion(td, dim, mults, H, ref["state"], dev, ks=ks)
    diff._engine(dev)
    eng = diff.model.engine(H, dev, training=True)
    eng.bind_train_schedule(diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod)
    big, small = eng.objective_plan(B), eng.objective_plan(9)
    assert _l(big, "FWD_ROWS")["grid"][0] == 8 and _l(small, "FWD_ROWS")["grid"][0] == 1
    x0, t, noise = (torch.from_numpy(a).to(dev) for a in ref["inputs"])
    t32 = t.to(torch.int32)
    _, saved_b = eng.objective_forward(x0, t32, noise, None, 2)
    xt_b, out_b = (v[:9].clone() for v in eng.objective_saved_views(saved_b, B))
    _, saved_s = eng.objective_forward(x0[:9].contiguous(), t32[:9].contiguous(), noise[:9].contiguous(), None, 2)
    xt_s, out_s = eng.objective_saved_views(saved_s, 9)
    torch.cuda.synchronize()
    assert torch.equal(xt_b, xt_s) and torch.equal(xt_s, diff.q_sample(x0[:9], t[:9], noise[:9]))
    out64 = ref["out64"][:9].numpy()
    e_route = max_abs(out_b.cpu().numpy(), out_s.cpu().numpy())
    e_b, e_s = max_abs(out_b.cpu().numpy(), out64), max_abs(out_s.cpu().numpy(), out64)
    print(f"\nrows 0..8 of the fused forward at B=250 vs B=9: outputs differ by {e_route:.2e} (vs float64: {e_b:.2e} / {e_s:.2e})")
    assert e_route <= TOL_STEP and e_b <= TOL_STEP and e_s <= TOL_STEP
