"""The backward pass at the batch sizes training runs (the benchmarked PointMaze step is batch 256, the reference's
train.py defaults to 128), where the host planner (csrc/host_plan.hpp: wgrad_geom, choose_tile, plan_split) picks
other kernels and other control flow than at the batches of 9 and less of tests/test_hip_train.py:

  conv_wgrad        several staged chunks per block: the double-buffered steady state (fetch chunk i + 1 into the other
                    LDS stage while chunk i is computed), the `nb + smp < s_hi` tail of a part-filled chunk behind full
                    ones, the windowed halo across the windows of several samples in one block
  sum_slabs         more than 8 slabs (its two-slab loop), slab counts that give the four thread groups unequal trips
  col_sums_many     its unrolled loop (batch >= 25) with a tail
  conv GEMMs        data-gradient and training-forward launches on tiles 1 / 2 / 8 with and without grid split-K

(a) test_large_batch_gradients_vs_float64: every parameter gradient, d loss / d x_t, the loss and the training
    forward's output against the oracle in float64 (oracle.denoiser on cast_weights(w, float64)), the fp32 oracle's own
    distance printed beside the engine's; a second call bit for bit equal.
(b) test_planner_knobs_on_reference_gradients: the reference's own gradient fixtures again under wgrad_blocks in
    {1, 8, 64, 4096} and forced conv tiles.
(c) test_large_batch_rows_match_small_batch_route: rows 0..8 of a batch-256 call against the batch-9 call.
(d) every case asks Engine.backward_plan (dad_debug_backward_plan: host logic only) which path it takes BEFORE it runs
    and asserts the property it exists for; test_matrix_reaches_every_backward_path asserts the coverage of the whole
    matrix without a device, so a retuned planner that lets a case fall back to one chunk per block fails the CPU suite.

Gates (none new): gradients |g_hip - g_f64| <= 2e-5 max|g_f64| per tensor (REL of test_hip_train.py, scales by
tests/util.py::grad_scales); training-forward output <= TOL_STEP (5e-6) from the float64 forward; loss 2e-6 relative.
The fp32 oracle itself was 1.2e-6 .. 2.8e-6 max|g| from float64 on five of these shapes when the gate was chosen.

Measured on an MI355X (`-s` prints every case): (a) engine 0.8e-6 .. 2.0e-6 max|g| from float64 (worst: d x_t of
c2048_B96), the fp32 oracle 1.4e-6 .. 3.9e-6; outputs 0.9e-6 .. 1.6e-6; (b) worst 4.7e-6 (grads_tiny_k3, forced tile 2);
(c) 1.4e-6.  The engine accepts and passes batch 512.  Each of three deliberate one-line errors made cases of (a) fail
while tests/test_hip_train.py kept passing: conv_wgrad always computing from LDS stage 0 (10 cases of (a), 11 of (b):
wgrad_blocks 1 / 8 / 64), sum_slabs_kernel stepping by 16 slabs (all 11 of (a)), col_sums_many_kernel without its
fourth chain (the 10 cases of (a) with a batch of 25 or more).
"""
import functools

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.golden.cases_long import LONG_GRAD_CASES, long_train_inputs
from tests.test_hip_long_horizon import _backward, _diffusion
from tests.test_hip_parity import TOL_STEP, build, dev  # noqa: F401  (dev: fixture)
from tests.test_hip_train import _loss_and_backward
from tests.util import as_torch, golden, grad_scales, max_abs, net_weights_torch

REL = 2e-5
T = 20
WGRAD_TAPS = (1, 3, 4, 5, 7)         # conv_wgrad instantiations (csrc/host_plan.hpp kWgradTaps)


# ------------------------------------------------------------------------------------------------ the matrix
def _combos(plan):
    """{(taps, tile, windowed): (launches, most chunks a block stages, launches with a part-filled last chunk behind
    full ones in their block)} of a backward plan."""
    out = {}
    for q in plan["launches"]:
        key = (q["taps"], q["tile"], bool(q["windowed"]))
        n, most, part = out.get(key, (0, 0, 0))
        out[key] = (n + 1, max(most, q["chunks"]), part + (q["samples"] % q["spc"] != 0 and q["last_chunks"] > 1))
    return out


def _convs(plan, which, cfg, split):
    return plan[which].get((cfg, split), 0)


# (a): (id, td, dim, mults, horizon, batch, kernel_size, wgrad_blocks or None, why, [(property, predicate on the plan)])
LARGE = [
    ("pointmaze_B256", 6, 128, (1, 2, 4), 32, 256, 5, None, "the benchmarked training step", [
        ("all 35 wgrad launches stage 2..8 chunks per block", lambda p: p["wgrads"] == 35 and p["multi"] == 35 and p["max_chunks"] == 8),
        ("64x64 / 64x32 tiles over several chunks in >= 21 launches",
         lambda p: sum(q["tile"] in (0, 1) and q["chunks"] > 1 for q in p["launches"]) >= 21),
        (">= 20 data-gradient convs on tile 1 without split-K", lambda p: _convs(p, "dgrad", 1, False) >= 20),
        (">= 15 training-forward convs on tile 1 without split-K", lambda p: _convs(p, "fwd", 1, False) >= 15),
        ("64 slabs in sum_slabs", lambda p: p["max_ksplit"] == 64),
    ]),
    ("pointmaze_B250", 6, 128, (1, 2, 4), 32, 250, 5, None, "part-filled last chunk behind full ones; ragged last conv tile; col_sums tail", [
        ("a part-filled last chunk in a multi-chunk block in >= 28 launches", lambda p: p["part_multi"] >= 28),
        ("... on each of the tiles 0, 1, 2", lambda p: all(any(k[1] == tile and v[2] for k, v in _combos(p).items()) for tile in (0, 1, 2))),
        ("63 slabs: both loops of sum_slabs and its tail, unequal trips", lambda p: p["max_ksplit"] == 63),
    ]),
    ("train_py_defaults_B128", 7, 32, (1, 2, 4, 8), 16, 128, 5, None, "the reference's train.py defaults (dim_mults, horizon 16, batch 128)", [
        ("four levels: 47 wgrad launches, up to 64 slabs", lambda p: p["wgrads"] == 47 and p["max_ksplit"] == 64),
        ("training-forward and data-gradient convs with and without split-K",
         lambda p: all(_convs(p, w, 0, s) >= 10 for w in ("fwd", "dgrad") for s in (False, True))),
    ]),
    ("halfcheetah_B32", 23, 256, (1, 4, 8), 32, 32, 5, None, "HalfCheetah widths: the 64x64 wgrad tile over up to 8 chunks", [
        (">= 27 launches over several chunks, up to 8, on tile 0", lambda p: p["multi"] >= 27 and p["max_chunks"] == 8 and
         any(q["tile"] == 0 and q["chunks"] == 8 for q in p["launches"])),
        ("3- and 4-tap wgrad on tile 0 over several chunks", lambda p: _combos(p)[(3, 0, False)][1] > 1 and _combos(p)[(4, 0, False)][1] > 1),
        ("training-forward convs on tiles 2 and 3 with split-K", lambda p: _convs(p, "fwd", 2, True) >= 8 and _convs(p, "fwd", 3, True) >= 8),
    ]),
    ("c2048_B96", 5, 256, (1, 8), 8, 96, 5, None, "2048 channels, 8 samples per chunk", [
        ("chunks of 8 and 16 samples, up to 6 per block",
         lambda p: p["max_chunks"] == 6 and {q["spc"] for q in p["launches"]} == {8, 16} and any(q["spc"] == 8 and q["chunks"] > 1 for q in p["launches"])),
        ("12 slabs", lambda p: p["max_ksplit"] == 12),
    ]),
    ("tiny_B512", 6, 32, (1, 2, 4), 32, 512, 5, None, "beyond 256: col_sums 16 trips, deep slab sums on narrow layers", [
        ("256 slabs", lambda p: p["max_ksplit"] == 256),
        ("the 32x32 tile over 4 chunks", lambda p: _combos(p)[(5, 2, False)][1] == 4),
    ]),
    ("H256_B96", 6, 32, (1, 2, 4), 256, 96, 5, None, "windowed wgrad over several chunks per block", [
        ("9 windowed launches, 1- and 5-tap ones over 2 chunks",
         lambda p: p["windowed"] == 9 and all(_combos(p)[k][1] >= 2 for k in ((1, 3, True), (5, 2, True), (5, 3, True)))),
        ("training-forward and data-gradient convs on the 128-position tile without split-K",
         lambda p: _convs(p, "fwd", 8, False) >= 9 and _convs(p, "dgrad", 8, False) >= 12),
    ]),
    ("H256_B24_wb16", 6, 32, (1, 2, 4), 256, 24, 5, 16, "windows of different samples in one block (wgrad_blocks 16)", [
        ("every windowed instantiation over >= 3 chunks (= windows) per block", lambda p: all(v[1] >= 3 for k, v in _combos(p).items() if k[2])),
        ("every windowed block walks across the windows of more than one sample",
         lambda p: all(q["sps"] > q["samples"] // 24 for q in p["launches"] if q["windowed"])),
        ("the 128-position tile with split-K", lambda p: _convs(p, "fwd", 8, True) >= 1 and _convs(p, "dgrad", 8, True) >= 1),
    ]),
    ("k3_B512", 6, 64, (1, 2, 4), 32, 512, 3, None, "TemporalUnet(kernel_size=3): wgrad<3> in the steady state", [
        ("every 3-tap instantiation over several chunks", lambda p: all(v[1] > 1 for k, v in _combos(p).items() if k[0] == 3)),
        ("the unaligned 3-tap launch among them", lambda p: _combos(p)[(3, 3, False)][1] > 1),
    ]),
    ("k7_B250_wb16", 7, 32, (1, 4), 16, 250, 7, 16, "kernel_size 7: wgrad<7> in the steady state (wgrad_blocks 16)", [
        ("every 7-tap instantiation over several chunks", lambda p: all(v[1] > 1 for k, v in _combos(p).items() if k[0] == 7)),
        ("the unaligned tile with a part-filled last chunk behind full ones", lambda p: any(k[1] == 3 and v[2] for k, v in _combos(p).items())),
    ]),
    ("d96_H24_B128", 6, 96, (1, 2, 4), 24, 128, 5, None, "padded widths and a padded horizon: zero rows and masked groups inside multi-chunk blocks", [
        (">= 32 launches over several chunks", lambda p: p["multi"] >= 32),
        ("training-forward convs on tile 1 with split-K", lambda p: _convs(p, "fwd", 1, True) >= 8),
    ]),
]

# (b): the reference's own gradient fixtures under the planner's knobs
KNOB_FIXTURES = ["grads_tiny", "grads_tiny4", "grads_pointmaze_B9", "grads_tiny_k3", "grads_tiny_k7", "grads_tiny_d48",
                 "grads_tiny_H256"]
KNOBS = [("wgrad_blocks", 1), ("wgrad_blocks", 8), ("wgrad_blocks", 64), ("wgrad_blocks", 4096),
         ("tile", 1), ("tile", 2), ("tile", 99)]
KNOB_CASES = [(f, k, v) for f in KNOB_FIXTURES for k, v in KNOBS + ([("tile", 8), ("tile", 9)] if f == "grads_tiny_H256" else [])]


def _fixture_case(name):
    """(net, horizon, T, batch, loss type, predict_epsilon, weighted) of a gradient fixture."""
    for c in cases.GRAD_CASES:
        if c[0] == name:
            return c[1], cases.H, c[2], c[3], c[4], c[5], c[6]
    for c in LONG_GRAD_CASES:
        if c[0] == name:
            return c[1], c[2], c[3], c[4], c[5], c[6], False
    raise KeyError(name)


def _knob_properties(name, knob, value):
    """What a knob case exists for, as [(property, predicate on the plan)]."""
    if knob == "wgrad_blocks" and value == 1:
        props = [("one block per tile, no slab sum, several chunks per block",
                  lambda p: p["max_ksplit"] == 1 and p["multi"] >= 1 and all(q["chunks"] * q["spc"] >= q["samples"] for q in p["launches"]))]
        if name == "grads_pointmaze_B9":
            props.append(("up to 5 chunks per block with a part-filled last one", lambda p: p["max_chunks"] >= 5 and p["part_multi"] >= 1))
        if name == "grads_tiny_H256":
            props.append(("12 windows per block", lambda p: any(q["windowed"] and q["chunks"] == 12 for q in p["launches"])))
        return props
    if knob == "wgrad_blocks" and value in (8, 64):
        return [("mixed splits: the launches split the batch to different depths",
                 lambda p: p["max_ksplit"] > 1 and len({q["ksplit"] for q in p["launches"]}) > 1)]
    if knob == "wgrad_blocks":
        return [("one chunk per block everywhere: the deepest slab sums",
                 lambda p: p["multi"] == 0 and all(q["ksplit"] * q["spc"] >= q["samples"] for q in p["launches"]))]
    if value == 99:
        return [("no conv launch splits K over the grid", lambda p: not any(s for w in ("fwd", "dgrad") for (_, s) in p[w]))]
    return [(f"training-forward and data-gradient convs on tile {value}",
             lambda p: sum(n for (c, _), n in p["fwd"].items() if c == value) >= 1 and sum(n for (c, _), n in p["dgrad"].items() if c == value) >= 1)]


def _host_engine(td, dim, mults, H, ks, time_dim=None):
    """An engine that was created but holds no weights: enough to plan (no device call)."""
    from dynamics_aware_diffusion_amd._engine import HipEngine
    return HipEngine(transition_dim=td, dim=dim, channels=[dim * k for k in mults], horizon=H, n_timesteps=T, time_dim=time_dim,
                     kernel_size=ks, training=True)


def _set_knob(eng, knob, value):
    """Through the library directly: Engine.debug_set_* enter the device's context, which the CPU suite has not."""
    from dynamics_aware_diffusion_amd._engine import _check
    if knob == "wgrad_blocks":
        _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, b"wgrad_blocks", int(value)))
    else:
        _check(eng.lib, eng.lib.dad_debug_set_tile(eng._h, int(value)))


def _assert_path(label, plan, props):
    for text, pred in props:
        assert pred(plan), f"{label}: the planner no longer gives '{text}': " \
                           f"{ {k: v for k, v in plan.items() if k != 'launches'} } {sorted(_combos(plan).items())}"
    return "; ".join(text for text, _ in props)


def _matrix_plans():
    """(label, batch, plan) of every case of (a) and (b), planned on the host."""
    out = []
    for name, td, dim, mults, H, B, ks, wb, _, props in LARGE:
        eng = _host_engine(td, dim, mults, H, ks)
        if wb is not None:
            _set_knob(eng, "wgrad_blocks", wb)
        out.append((name, B, eng.backward_plan(B), props))
    for name, knob, value in KNOB_CASES:
        net, H, _, B, _, _, _ = _fixture_case(name)
        _, _, td, dim, mults = cases.net_dims(net)
        eng = _host_engine(td, dim, mults, H, cases.net_kernel_size(net), cases.net_time_dim(net))
        _set_knob(eng, knob, value)
        out.append((f"{name}[{knob}={value}]", B, eng.backward_plan(B), _knob_properties(name, knob, value)))
    return out


def test_matrix_reaches_every_backward_path():
    """No device needed: the cases of (a) and (b) together reach what the module exists for.  Each case's own
    property is asserted too, so a planner change that lets one fall back names the case here."""
    plans = _matrix_plans()
    assert len(plans) == len(LARGE) + len(KNOB_CASES) == 11 + 7 * 7 + 2
    for label, _, plan, props in plans:
        _assert_path(label, plan, props)
    combos = {}                 # (taps, tile, windowed) -> (most chunks per block, cases with a part-filled chunk behind full ones)
    for label, _, plan, _ in plans:
        for key, (n, most, part) in _combos(plan).items():
            a, b = combos.get(key, (0, 0))
            combos[key] = (max(a, most), b + (part > 0))
    # every tap count the library has, every tile (3: rows that are not whole float4s, the trajectory's columns), windowed
    assert {k[0] for k in combos} == set(WGRAD_TAPS)
    assert {k[1] for k in combos} == {0, 1, 2, 3}
    assert any(k[2] for k in combos)
    # whatever instantiation the matrix launches at all runs its steady state (>= 2 chunks per block) somewhere
    single = sorted(k for k, v in combos.items() if v[0] < 2)
    assert not single, f"(taps, tile, windowed) launched with one chunk per block only: {single}"
    for tile in range(4):
        assert any(k[1] == tile and v[1] for k, v in combos.items()), f"no part-filled last chunk behind full ones on tile {tile}"
    # sum_slabs_kernel: >= 13 slabs with a remainder mod 8 other than 0 / 4: both loops, the tail, unequal trips per group
    ksplits = {q["ksplit"] for _, _, plan, _ in plans for q in plan["launches"]}
    assert any(k >= 13 and k % 8 not in (0, 4) for k in ksplits), sorted(ksplits)
    # col_sums_many_kernel: the unrolled loop (b + 24 < B) plus its tail
    assert any(B >= 57 and B % 32 != 0 for _, B, _, _ in plans)
    # conv GEMMs of the training forward and of the data gradients: tiles 0, 1, 2 and the 128-position tile 8, each with
    # and without grid split-K
    for which in ("fwd", "dgrad"):
        seen = set()
        for _, _, plan, _ in plans:
            seen |= set(plan[which])
        missing = [(cfg, s) for cfg in (0, 1, 2, 8) for s in (False, True) if (cfg, s) not in seen]
        assert not missing, f"{which}: no launch on (tile, split-K) {missing}"


def test_backward_plan_needs_training_and_a_batch():
    from dynamics_aware_diffusion_amd._engine import DadError, HipEngine
    eng = HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=T)
    with pytest.raises(DadError, match="dad_model_set_training"):
        eng.backward_plan(4)
    eng = _host_engine(6, 32, (1, 2, 4), 32, 5)
    with pytest.raises(DadError):
        eng.backward_plan(0)
    p = eng.backward_plan(4)
    assert p["wgrads"] == len(p["launches"]) == 35 and sum(p["tile"]) == 35 and sum(p["taps_tile"].values()) == 35
    assert sum(p["dgrad"].values()) == 39


# ------------------------------------------------------------------------------------------------ (a)
def _inputs(name, B, H, td):
    from dynamics_aware_diffusion_amd.utils import synth
    x0 = np.clip(synth.normal_like(20, f"tbatch.x.{name}", (B, H, td)) * 0.5, -1, 1).astype(np.float32)
    t = np.array([(3 * i + 1) % T for i in range(B)], dtype=np.int64)
    t[0], t[-1] = 0, T - 1                                       # both ends of the schedule
    noise = synth.normal_like(20, f"tbatch.n.{name}", (B, H, td))
    return x0, t, noise


def _train_step(diff, x0, t, noise, dev, reduce="mean"):
    """As _backward of test_hip_long_horizon.py, keeping the training forward's output: (loss, out, d x_t, gradients)."""
    for p in diff.parameters():
        p.grad = None
    x0t, tt, nz = torch.from_numpy(x0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(noise).to(dev)
    with torch.enable_grad():
        x_t = diff.q_sample(x0t, tt, nz).detach().requires_grad_(True)
        out = diff.model(x_t, tt)
        per = diff.loss_fn(out, nz)
        loss = per.mean() if reduce == "mean" else per.sum()
        loss.backward()
    torch.cuda.synchronize()
    return (float(loss), out.detach().cpu().numpy(), x_t.grad.cpu().numpy(),
            {k: p.grad.detach().cpu().numpy().copy() for k, p in diff.model.named_parameters()})


@functools.lru_cache(maxsize=None)
def _large_oracle(name):
    """The weights, the draws and the float64 oracle of a case of LARGE, computed once per run (this module and
    tests/test_hip_objective_batch.py both ask): state, (x0, t, noise), loss / gradients / d x_t / output in float64,
    and the fp32 oracle's own distance from them (per gradient on the scale of grad_scales, d x_t, output).  Nobody
    writes into what this returns."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    _, td, dim, mults, H, B, ks, _, _, _ = next(c for c in LARGE if c[0] == name)
    state = synth.synth_unet_state(td, dim, mults, seed=41, affine_jitter=0.3, kernel_size=ks)
    x0, t, noise = _inputs(name, B, H, td)
    w = as_torch(state)
    sched = orc.schedule_buffers("cosine", T)
    x0t, tt, nz = torch.from_numpy(x0), torch.from_numpy(t), torch.from_numpy(noise)
    w64 = orc.cast_weights(w, torch.float64)
    s64 = {k: v.double() for k, v in sched.items()}
    l64, g64, dx64 = orc.training_gradients(w64, s64, x0t.double(), tt, nz.double())
    _, _, out64 = orc.training_loss(w64, s64, x0t.double(), tt, nz.double())
    l32, g32, dx32 = orc.training_gradients(w, sched, x0t, tt, nz)               # only to print its own distance
    _, _, out32 = orc.training_loss(w, sched, x0t, tt, nz)
    scales = grad_scales(g64)
    orc_errs = {k: max_abs(g32[k].numpy(), g64[k].numpy()) / scales[k] for k in g64}
    orc_errs["d x_t"] = max_abs(dx32.numpy(), dx64.numpy()) / float(dx64.abs().max())
    return {"state": state, "inputs": (x0, t, noise), "l64": l64, "g64": g64, "dx64": dx64, "out64": out64, "scales": scales,
            "orc_errs": orc_errs, "o_out": max_abs(out32.numpy(), out64.numpy())}


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE, ids=lambda c: c[0])
def test_large_batch_gradients_vs_float64(case, dev):
    name, td, dim, mults, H, B, ks, wb, why, props = case
    ref = _large_oracle(name)
    state = ref["state"]
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, state, dev, ks=ks)
    eng = diff.model.engine(H, dev, training=True)
    if wb is not None:
        eng.debug_set_option("wgrad_blocks", wb)
    path = _assert_path(name, eng.backward_plan(B), props)
    x0, t, noise = ref["inputs"]
    loss, out, dx, grads = _train_step(diff, x0, t, noise, dev)
    loss2, out2, dx2, grads2 = _train_step(diff, x0, t, noise, dev)
    assert diff.model._engine is eng, "the engine was rebuilt: the plan asserted above is not the one that ran"

    l64, g64, dx64, out64, scales, orc_errs, o_out = (ref[k] for k in ("l64", "g64", "dx64", "out64", "scales", "orc_errs", "o_out"))
    assert set(grads) == set(g64)
    errs = {k: max_abs(grads[k], g64[k].numpy()) / scales[k] for k in grads}
    errs["d x_t"] = max_abs(dx, dx64.numpy()) / float(dx64.abs().max())
    worst = max(errs, key=errs.get)
    oworst = max(orc_errs, key=orc_errs.get)
    e_out = max_abs(out, out64.numpy())
    e_loss = abs(loss - float(l64)) / max(1.0, abs(float(l64)))
    print(f"\n{name} ({why})\n  path: {path}\n  gradients vs float64, x max|g|: engine {errs[worst]:.2e} ({worst}), d x_t {errs['d x_t']:.2e}; "
          f"fp32 oracle {orc_errs[oworst]:.2e} ({oworst}), d x_t {orc_errs['d x_t']:.2e}\n"
          f"  training-forward output vs float64: engine {e_out:.2e}, fp32 oracle {o_out:.2e}; loss: engine {e_loss:.1e} relative")
    for k in grads:
        assert np.isfinite(grads[k]).all(), k
    bad = {k: f"{e:.2e}" for k, e in errs.items() if not e <= REL}
    assert not bad, f"{name}: gradients farther than {REL} x max|g| from float64: {bad}"
    assert e_out <= TOL_STEP, f"{name}: training-forward output {e_out:.2e} from the float64 forward"
    assert e_loss <= 2e-6, f"{name}: loss {loss} vs {float(l64)}"
    # fixed-order reductions and ordered staging: a second call gives the same bits
    assert loss == loss2 and np.array_equal(out, out2) and np.array_equal(dx, dx2)
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), f"{name}: {k} differs between two calls"


# ------------------------------------------------------------------------------------------------ (b)
@functools.lru_cache(maxsize=2)
def _fixture_oracle(name):
    from oracle import denoiser as orc
    net, H, Tn, B, loss_type, pred_eps, weighted = _fixture_case(name)
    if H == cases.H:
        x0, t, noise, wts = cases.train_inputs(name, net, Tn, B, weighted)
    else:
        (x0, t, noise), wts = long_train_inputs(name, net, H, Tn, B), None
    _, og, odx = orc.training_gradients(net_weights_torch(net), orc.schedule_buffers("cosine", Tn), torch.from_numpy(x0),
                                        torch.from_numpy(t), torch.from_numpy(noise), loss_type, pred_eps,
                                        None if wts is None else torch.from_numpy(wts))
    return {k: v.numpy() for k, v in og.items()}, odx.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", KNOB_CASES, ids=lambda c: f"{c[0]}-{c[1]}{c[2]}")
def test_planner_knobs_on_reference_gradients(case, dev):
    """Assertions and tolerance of test_parameter_gradients_vs_reference (sampled elements against the fixture, every
    element against the oracle, the sums), d loss / d x_t for the long-horizon fixture as its own test holds it."""
    name, knob, value = case
    net, H, Tn, B, loss_type, pred_eps, weighted = _fixture_case(name)
    g = golden(name)
    if H == cases.H:
        diff = build(net, Tn, "cosine", dev, loss_type=loss_type, predict_epsilon=pred_eps)
    else:
        od, ad, td, dim, mults = cases.net_dims(net)
        diff = _diffusion(td, od, ad, dim, mults, H, Tn, cases.net_weights(net), dev, loss_type=loss_type, predict_epsilon=pred_eps)
    if H == cases.H:
        diff._engine(dev)                      # diff.loss() binds the schedule to the denoiser: do it before the engine is taken
    eng = diff.model.engine(H, dev, training=True)
    try:
        if knob == "wgrad_blocks":
            eng.debug_set_option("wgrad_blocks", value)
        else:
            eng.debug_set_tile(value)
        path = _assert_path(f"{name}[{knob}={value}]", eng.backward_plan(B), _knob_properties(name, knob, value))
        dx = None
        if H == cases.H:
            loss = float(_loss_and_backward(diff, name, net, Tn, B, weighted, dev))
            grads = {k: p.grad.detach().cpu().numpy() for k, p in diff.model.named_parameters()}
        else:
            x0, t, noise = long_train_inputs(name, net, H, Tn, B)
            loss, dx, grads = _backward(diff, x0, t, noise, loss_type, dev)
        assert diff.model._engine is eng
    finally:
        eng.debug_set_option("wgrad_blocks", 256)
        eng.debug_set_tile(-1)
    assert abs(loss - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    og, odx = _fixture_oracle(name)
    assert set(grads) == set(og)
    worst, worst_key = 0.0, None
    for k, got in grads.items():
        assert np.isfinite(got).all(), k
        scale = max(float(g["max." + k]), 1e-12)
        flat = got.reshape(-1)
        idx = cases.grad_sample_index(flat.size)
        e_ref = float(np.max(np.abs(flat[idx].astype(np.float64) - g["g." + k]))) / scale      # the reference itself
        e_orc = max_abs(got, og[k]) / scale                                                     # every element
        e_sum = abs(float(flat.astype(np.float64).sum()) - float(g["sum." + k])) / (scale * max(1.0, np.sqrt(flat.size)))
        if max(e_ref, e_orc) > worst:
            worst, worst_key = max(e_ref, e_orc), k
        assert e_ref <= REL and e_orc <= REL, f"{k}: rel err vs reference {e_ref:.2e}, vs oracle {e_orc:.2e}"
        assert e_sum <= REL, f"{k}: sum of the gradient off by {e_sum:.2e} (relative to max|g| sqrt(n))"
    e_dx = 0.0
    if dx is not None:
        e_dx = max(max_abs(dx, g["dx"]), max_abs(dx, odx)) / float(np.abs(g["dx"]).max())
        assert e_dx <= REL
    print(f"\n{name} {knob}={value}: {path}\n  worst parameter-gradient error vs the reference's fixture / the oracle "
          f"{worst:.2e} x max|g| ({worst_key})" + (f", d x_t {e_dx:.2e}" if dx is not None else ""))


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.gpu
def test_large_batch_rows_match_small_batch_route(dev):
    """With the loss a SUM the rows are independent: d loss / d x_t of rows 0..8 of a batch-256 call (conv tiles 1,
    no split-K) equals the same rows run as a batch of 9 (tile 0 under grid split-K), to the gate of (a) on the scale
    of the float64 oracle's gradient for those rows."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    name, td, dim, mults, H, B, ks, _, _, _ = LARGE[0]
    state = synth.synth_unet_state(td, dim, mults, seed=41, affine_jitter=0.3, kernel_size=ks)
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, state, dev, ks=ks)
    eng = diff.model.engine(H, dev, training=True)
    big, small = eng.backward_plan(B), eng.backward_plan(9)
    assert _convs(big, "dgrad", 1, False) >= 20 and not any(c == 1 for c, _ in small["dgrad"])
    x0, t, noise = _inputs(name, B, H, td)
    _, out_b, dx_b, _ = _train_step(diff, x0, t, noise, dev, reduce="sum")
    _, out_s, dx_s, _ = _train_step(diff, x0[:9], t[:9], noise[:9], dev, reduce="sum")
    w64 = orc.cast_weights(as_torch(state), torch.float64)
    s64 = {k: v.double() for k, v in orc.schedule_buffers("cosine", T).items()}
    _, _, dx64 = orc.training_gradients(w64, s64, torch.from_numpy(x0[:9]).double(), torch.from_numpy(t[:9]),
                                        torch.from_numpy(noise[:9]).double())
    dx64 = dx64.numpy() * (9 * H * td)                          # the oracle's loss is a mean over these rows
    scale = float(np.abs(dx64).max())
    e_route = max_abs(dx_b[:9], dx_s) / scale
    e_b, e_s = max_abs(dx_b[:9], dx64) / scale, max_abs(dx_s, dx64) / scale
    print(f"\nrows 0..8 of B=256 vs B=9: d x_t differs by {e_route:.2e} x max|g| (vs float64: {e_b:.2e} / {e_s:.2e}); "
          f"outputs differ by {max_abs(out_b[:9], out_s):.2e}")
    assert e_route <= REL and e_b <= REL and e_s <= REL
    assert max_abs(out_b[:9], out_s) <= TOL_STEP
