"""The library guide on the GPU: ``guide_mlp_kernel`` (csrc/guide_mlp.hpp) through ``GuideState`` and the fused guided
loop ``dad_guided_loop`` through ``HipEngine`` and ``ValueGuidedPolicy.fused_guide``.

1. gradient and per-row value against float64 autograd of the same module, gated by the module's own fp32 distance;
2. the reference's guided fixtures through the library route;
3. the fused guided loop bit for bit against the Python-driven loop fed by the same kernel (the test of launch order);
4. weights changed in place are followed, under graph replay too;
5. get_action / get_actions with fused_guide and use_graph against the stepwise route.

Section 1 prints, per case, the kernel's error, the module's own fp32 error e32 and their ratio (``pytest -s``).
"""
import functools
import math
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.golden import cases
from tests.test_hip_parity import TOL_LOOP, build, dev, injected_noise  # noqa: F401  (dev: fixture)
from tests.util import as_torch, golden, max_abs

pytestmark = pytest.mark.gpu

ACTS = {"tanh": nn.Tanh, "relu": nn.ReLU, "mish": nn.Mish}
# (id, in_dim, widths, transition_dim); the last has in_dim == td: no channel is left for the zero fill
GRAD_NETS = [
    ("4-16-1", 4, (16, 1), 6),
    ("17-33-1", 17, (33, 1), 23),
    ("6-256-256-1", 6, (256, 256, 1), 8),
    ("11-64-64-64-1", 11, (64, 64, 64, 1), 14),
    ("39-512-512-1", 39, (512, 512, 1), 67),
    ("9-24-1-td9", 9, (24, 1), 9),
]
GRAD_ROWS = ((1, 8), (4, 8), (3, 11))       # 8 rows, exactly 32, 33 (a second block with one row)
KINK_BAND, KINK_CAP = 1e-6, 0.05


def value_module(in_dim, widths, act, seed=41, name="guide"):
    """nn.Sequential of the net with torch's default init range scaled by 1.7 and biases U(-0.7, 0.7), from synth."""
    from dynamics_aware_diffusion_amd.utils import synth
    mods, k = [], in_dim
    for i, n in enumerate(widths):
        lin = nn.Linear(k, n)
        tag = f"{name}.{in_dim}.{'-'.join(map(str, widths))}.{i}"
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(synth.uniform(seed, tag + ".w", (n, k), 1.7 / math.sqrt(k))))
            lin.bias.copy_(torch.from_numpy(synth.uniform(seed, tag + ".b", (n,), 0.7)))
        mods.append(lin)
        if i + 1 < len(widths):
            mods.append(ACTS[act]())
        k = n
    return nn.Sequential(*mods)


def autograd_reference(module, x, in_dim, dtype):
    """(gradient of the sum of the values (B, H, td), values (B, H), hidden pre-activations) in ``dtype`` on the CPU."""
    m = module.to(dtype)
    probe = x.to(dtype).clone().requires_grad_(True)
    with torch.enable_grad():
        pre, h = [], probe[..., :in_dim]
        for mod in m:
            h = mod(h)
            if isinstance(mod, nn.Linear):
                pre.append(h.detach())
        (g,) = torch.autograd.grad(h.sum(), probe)
    return g, h.detach().squeeze(-1), pre[:-1]


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("net", GRAD_NETS, ids=lambda n: n[0])
def test_gradient_and_value_against_float64(net, act, dev):
    """Gate per case, in units of max|g| (max|V|): 4 x max(e32, 2^-22), e32 the distance of the same module's fp32 torch
    autograd on the CPU from float64 on the same inputs.  ReLU rows with a hidden pre-activation inside the kink band
    (|a| < 1e-6 max|a| of its layer, float64) are left out: at most 5 % of the rows, rounded up to one, asserted on the
    reference alone."""
    from dynamics_aware_diffusion_amd import _engine
    from dynamics_aware_diffusion_amd.utils import synth
    name, in_dim, widths, td = net
    module = value_module(in_dim, widths, act)
    plan = _engine.guide_plan(in_dim, widths, act, 4, 8, td)
    if name == "39-512-512-1" and act == "mish":
        assert plan["refused"] == "lds" and plan["lds_bytes"] > 160 * 1024
        state, why = _engine.GuideState.compile(module.to(dev), in_dim, dev)
        assert state is None and "lds" in why
        return
    assert plan["refused"] is None
    dev_module = value_module(in_dim, widths, act).to(dev)
    state, why = _engine.GuideState.compile(dev_module, in_dim, dev)
    assert state is not None, why
    worst = 0.0
    for B, H in GRAD_ROWS:
        q = state.plan(B, H, td)
        assert q["refused"] is None and q["grid"] == (B * H + 31) // 32 and q["lds_bytes"] <= 160 * 1024
        x = torch.from_numpy(synth.normal_like(43, f"guide.x.{name}.{B}.{H}", (B, H, td)))
        g64, v64, pre = autograd_reference(value_module(in_dim, widths, act), x, in_dim, torch.float64)
        g32, v32, _ = autograd_reference(value_module(in_dim, widths, act), x, in_dim, torch.float32)
        keep = torch.ones(B, H, dtype=torch.bool)
        if act == "relu":
            for a in pre:
                keep &= ~(a.abs() < KINK_BAND * a.abs().max()).any(dim=-1)
            assert int((~keep).sum()) <= max(1, math.ceil(KINK_CAP * B * H)), (name, B, H, int((~keep).sum()))
        got_g, got_v = state.grad(x.to(dev), value_rows=True)
        torch.cuda.synchronize()
        got_g, got_v = got_g.cpu().double(), got_v.cpu().double()
        assert torch.isfinite(got_g).all() and torch.isfinite(got_v).all()
        assert not got_g[..., in_dim:].any(), "channels the guide does not read must get a zero gradient"
        gs, vs = float(g64[keep].abs().max()), float(v64[keep].abs().max())
        e32_g = float((g32.double() - g64)[keep].abs().max()) / gs
        e32_v = float((v32.double() - v64)[keep].abs().max()) / vs
        err_g = float((got_g - g64)[keep].abs().max()) / gs
        err_v = float((got_v - v64)[keep].abs().max()) / vs
        print(f"\nguide {name} {act} B={B} H={H}: grad err {err_g:.2e} (e32 {e32_g:.2e}, ratio {err_g / max(e32_g, 1e-30):.2f}), "
              f"value err {err_v:.2e} (e32 {e32_v:.2e}, ratio {err_v / max(e32_v, 1e-30):.2f}), left out {int((~keep).sum())}")
        worst = max(worst, err_g / max(e32_g, 2.0 ** -22), err_v / max(e32_v, 2.0 ** -22))
        assert err_g <= 4 * max(e32_g, 2.0 ** -22), (name, act, B, H, err_g, e32_g)
        assert err_v <= 4 * max(e32_v, 2.0 ** -22), (name, act, B, H, err_v, e32_v)
    print(f"guide {name} {act}: worst error / max(e32, 2^-22) = {worst:.2f}")


# ------------------------------------------------------------------------------------------------ reference fixtures
def _value_sequential(od_dim, dev):
    vw = as_torch(cases.value_net_weights(od_dim))
    seq = nn.Sequential(nn.Linear(od_dim, cases.VALUE_HIDDEN), nn.Tanh(), nn.Linear(cases.VALUE_HIDDEN, 1))
    with torch.no_grad():
        seq[0].weight.copy_(vw["w1"]); seq[0].bias.copy_(vw["b1"])
        seq[2].weight.copy_(vw["w2"]); seq[2].bias.copy_(vw["b2"])
    return seq.to(dev)


def _count_calls(eng, counts):
    """Count the engine calls of one loop on this engine object (restored by the caller's finally)."""
    saved = {}
    for name in ("guided_loop", "denoise_step", "sampler_step"):
        fn = getattr(eng, name)
        saved[name] = fn

        def wrapped(*a, _fn=fn, _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return _fn(*a, **kw)
        setattr(eng, name, wrapped)
    return saved


@pytest.mark.parametrize("case", [c[:2] + (c[2], c[2]) + c[3:] for c in cases.GUIDE_CASES] + list(cases.GUIDE_SHORT_CASES),
                         ids=lambda c: c[0])
def test_reference_fixtures_through_the_library_route(case, dev):
    from dynamics_aware_diffusion_amd import ValueGuidedPolicy
    name, net, T, n_steps, B, gw = case
    g = golden(name)
    diff = build(net, T, "cosine", dev)
    keep = diff.n_timesteps
    diff.n_timesteps = n_steps
    eng = diff._engine(dev)
    counts = {}
    saved = _count_calls(eng, counts)
    try:
        pol = ValueGuidedPolicy(diff, None, _value_sequential(diff.observation_dim, dev), guide_weight=gw)
        pol.fused_guide = True
        cond = {0: torch.from_numpy(cases.loop_condition(name, net)).to(dev)}
        assert pol.guide_route(cond, B)[0] == "library", pol.guide_route(cond, B)
        noise = cases.loop_noise(name, net, n_steps, B)
        with injected_noise(noise, dev):
            x = pol.sample_loop(batch_size=B, conditions=cond)
        torch.cuda.synchronize()
    finally:
        diff.n_timesteps = keep
        for k, fn in saved.items():
            delattr(eng, k)
    assert counts == {"guided_loop": 1}, counts
    err = max_abs(x.cpu().numpy(), g["x_final"])
    print(f"\n{name}: library route max|x_final - reference| = {err:.2e}")
    assert err <= TOL_LOOP


# ------------------------------------------------------------------------------------------------ launch order
LOOP_T, LOOP_GW = 20, 0.7
# (id, dim, mults, horizon, batch, cc option, what the plans must say)
LOOP_NETS = [
    ("tiny_B3", 32, (1, 2, 4), 32, 3, None),                  # the small-batch kernels
    ("d64_m1_H16_B893", 64, (1,), 16, 893, 0),                # the batch kernels with the seam taken, a full chip of blocks
]
LOOP_TD, LOOP_OD = 6, 5


@functools.lru_cache(maxsize=None)
def _loop_inputs(name):
    from dynamics_aware_diffusion_amd.utils import synth
    _, dim, mults, H, B, _ = next(n for n in LOOP_NETS if n[0] == name)
    return {"state": synth.synth_unet_state(LOOP_TD, dim, mults, seed=59, affine_jitter=0.3),
            "noise": torch.from_numpy(synth.normal_like(61, f"guide.loop.noise.{name}", (2, 6, B, H, LOOP_TD))),
            "cond": torch.from_numpy(synth.uniform(61, f"guide.loop.cond.{name}", (B, LOOP_TD), 0.9))}


@functools.lru_cache(maxsize=None)
def _loop_setup(name):
    from tests.test_hip_long_horizon import _diffusion
    from dynamics_aware_diffusion_amd import _engine
    device = torch.device("cuda:0")
    _, dim, mults, H, B, cc = next(n for n in LOOP_NETS if n[0] == name)
    diff = _diffusion(LOOP_TD, LOOP_OD, 1, dim, mults, H, LOOP_T, _loop_inputs(name)["state"], device)
    eng = diff._engine(device)
    if cc is not None:
        eng.debug_set_option("cc", cc)
    small = eng.forward_plan(B)["small"]
    if cc is None:
        assert small, "batch 3 of the tiny net runs the small-batch kernels"
    else:
        assert not small and eng.seam_plan(B)["taken"], (eng.forward_plan(B)["small"], eng.seam_plan(B))
    state, why = _engine.GuideState.compile(value_module(LOOP_OD, (16, 1), "tanh", name="loopguide").to(device), LOOP_OD, device)
    assert state is not None, why
    return diff, eng, state


def _steps_of(diff, sampler, n_steps):
    """None (the ancestral steps) or the coefficient array of the strided sampler, in execution order."""
    if sampler == "ddpm":
        return None
    diff.set_sampler("ddim", steps=n_steps, eta=float(sampler[len("ddim"):]))
    try:
        arr = diff.sampler_plan()[0].copy()
    finally:
        diff.set_sampler("ddpm")
    return arr


def _start(inp, cond_mode, dev):
    x = inp["noise"][0, 0].to(dev).clone()
    cond = {"none": None, "shared": inp["cond"][:1], "rows": inp["cond"]}[cond_mode]
    if cond is not None:
        cond = cond.to(dev).contiguous()
        x[:, 0] = cond
    return x, cond


def _noise_kw(noise_mode, stack, seed, j=None):
    if noise_mode == "philox":
        return dict(seed=seed, row_offset=5) if j is None else dict(seed=seed, row_offset=5, draw=j + 1)
    return dict(noise_stack=stack) if j is None else dict(noise=stack[j])


def _fused(eng, state, arr, n_steps, x, cond, noise_mode, stack, seed, use_graph=False):
    kw = dict(cond0=cond, use_graph=use_graph, **_noise_kw(noise_mode, stack, seed))
    eng.guided_loop(x, state, LOOP_GW, steps=arr, n_steps=n_steps, **kw)


def _stepwise(eng, state, arr, n_steps, x, cond, noise_mode, stack, seed):
    for j in range(n_steps):
        kw = dict(cond0=cond, guide_grad=state.grad(x), guide_weight=LOOP_GW, **_noise_kw(noise_mode, stack, seed, j))
        if arr is None:
            eng.denoise_step(x, n_steps - 1 - j, **kw)
        else:
            eng.sampler_step(x, arr[j], **kw)


def _loop_cases(name):
    if name == "tiny_B3":
        return [(n, nm, cm) for n in (1, 2, 5) for nm in ("philox", "injected") for cm in ("none", "shared", "rows")]
    return [(n, nm, "rows") for n in (2, 5) for nm in ("philox", "injected")] + [(1, "philox", "none"), (5, "philox", "shared")]


@pytest.mark.parametrize("seam", (1, 0), ids=("seam", "noseam"))
@pytest.mark.parametrize("sampler", ("ddpm", "ddim0", "ddim0.5"))
@pytest.mark.parametrize("net", LOOP_NETS, ids=lambda n: n[0])
def test_fused_guided_loop_is_bit_equal_to_the_stepwise_loop(net, sampler, seam, dev):
    """A guide launch that reads x a launch too early, or a seam that finds the next step's gradient, shows as a
    difference; eager, and graph replay twice with two seeds (the second result against its own eager run)."""
    name = net[0]
    diff, eng, state = _loop_setup(name)
    inp = _loop_inputs(name)
    eng.debug_set_option("step_seam", seam)
    try:
        if net[5] is not None:
            assert eng.seam_plan(net[4])["taken"] == bool(seam)
        for n_steps, noise_mode, cond_mode in _loop_cases(name):
            arr = _steps_of(diff, sampler, n_steps)
            stacks = [inp["noise"][k, 1:1 + n_steps].to(dev).contiguous() for k in (0, 1)]
            seeds = (0x123456789ABCDEF, 77)
            want = []
            for k in (0, 1):
                x, cond = _start(inp, cond_mode, dev)
                _stepwise(eng, state, arr, n_steps, x, cond, noise_mode, stacks[k], seeds[k])
                want.append(x)
            x, cond = _start(inp, cond_mode, dev)
            _fused(eng, state, arr, n_steps, x, cond, noise_mode, stacks[0], seeds[0])
            torch.cuda.synchronize()
            assert torch.isfinite(x).all()
            assert torch.equal(x, want[0]), (name, sampler, seam, n_steps, noise_mode, cond_mode,
                                             float((x - want[0]).abs().max()))
            # graph: capture with the first seed / stack, replay with the second through the same buffers
            xg, zg = eng.persistent("test.guide.x", tuple(x.shape)), eng.persistent("test.guide.z", tuple(stacks[0].shape))
            for k in (0, 1):
                x0, cond = _start(inp, cond_mode, dev)
                xg.copy_(x0)
                zg.copy_(stacks[k])
                _fused(eng, state, arr, n_steps, xg, cond if cond is None else eng.persistent("test.guide.c", tuple(cond.shape)).copy_(cond),
                       noise_mode, zg, seeds[k], use_graph=True)
                torch.cuda.synchronize()
                assert torch.equal(xg, want[k]), (name, sampler, seam, n_steps, noise_mode, cond_mode, "graph", k,
                                                  float((xg - want[k]).abs().max()))
    finally:
        eng.debug_set_option("step_seam", 1)


def test_the_guide_changes_the_loop_and_zero_weight_is_the_unguided_loop(dev):
    diff, eng, state = _loop_setup("tiny_B3")
    inp = _loop_inputs("tiny_B3")
    outs = {}
    for gw in (LOOP_GW, 0.0, None):
        x, cond = _start(inp, "shared", dev)
        if gw is None:
            eng.sample_loop(x, 5, cond0=cond, seed=3)
        else:
            eng.guided_loop(x, state, gw, n_steps=5, cond0=cond, seed=3)
        torch.cuda.synchronize()
        outs[gw] = x.cpu()
    assert torch.equal(outs[0.0], outs[None])
    assert float((outs[LOOP_GW] - outs[None]).abs().max()) > 1e-4, "the guide left no trace in the result"


# ------------------------------------------------------------------------------------------------ weights in place
def test_weights_changed_in_place_are_followed(dev):
    from dynamics_aware_diffusion_amd import _engine
    diff, eng, _ = _loop_setup("tiny_B3")
    inp = _loop_inputs("tiny_B3")
    module = value_module(LOOP_OD, (16, 1), "tanh", name="inplace").to(dev)
    state, why = _engine.GuideState.compile(module, LOOP_OD, dev)
    assert state is not None, why
    xg = eng.persistent("test.guide.inplace", tuple(inp["noise"][0, 0].shape))
    results = {}
    for phase in ("before", "after"):
        if phase == "after":
            with torch.no_grad():
                for p in module.parameters():
                    p.mul_(-1.3)                        # bumps the versions
        x, cond = _start(inp, "shared", dev)
        g_module = state.grad(x)
        probe = x.clone().requires_grad_(True)
        with torch.enable_grad():
            (g_auto,) = torch.autograd.grad(module(probe[..., :LOOP_OD]).sum(), probe)
        assert float((g_module - g_auto).abs().max()) <= 1e-5 * float(g_auto.abs().max()), phase
        _stepwise(eng, state, None, 5, x, cond, "philox", None, 9)
        for use_graph in (False, True):
            x0, _ = _start(inp, "shared", dev)
            xg.copy_(x0)
            eng.guided_loop(xg, state, LOOP_GW, n_steps=5, cond0=cond, seed=9, row_offset=5, use_graph=use_graph)
            torch.cuda.synchronize()
            assert torch.equal(xg, x), (phase, use_graph, float((xg - x).abs().max()))
        results[phase] = x.cpu()
    assert not torch.equal(results["before"], results["after"])
    # a .data update moves no version: mark_changed() is the caller's word
    module[0].weight.data.mul_(0.5)
    stale = state.grad(_start(inp, "shared", dev)[0])
    state.mark_changed()
    fresh = state.grad(_start(inp, "shared", dev)[0])
    torch.cuda.synchronize()
    assert not torch.equal(stale, fresh)


# ------------------------------------------------------------------------------------------------ planner glue
def test_get_action_and_get_actions_take_the_library_route(dev):
    from dynamics_aware_diffusion_amd import ValueGuidedPolicy
    diff = build("tiny", 20, "cosine", dev)
    od, ad = diff.observation_dim, diff.action_dim
    norm = types.SimpleNamespace(
        obs_mean=np.linspace(-0.2, 0.3, od).astype(np.float32), obs_std=np.linspace(0.8, 1.3, od).astype(np.float32),
        action_mean=np.zeros(ad, np.float32), action_std=np.ones(ad, np.float32),
        normalize_observations=lambda o: (o - norm.obs_mean) / norm.obs_std,
        unnormalize_actions=lambda a: a * norm.action_std + norm.action_mean)
    obs = np.linspace(-0.5, 0.6, 3 * od).astype(np.float32).reshape(3, od)
    keep = (diff.sampler_rng, diff.seed, diff.use_graph)
    diff.sampler_rng, diff.seed = "philox", 21
    eng = diff._engine(dev)
    try:
        got = {}
        for fused in (False, True):
            pol = ValueGuidedPolicy(diff, norm, _value_sequential(od, dev), guide_weight=0.5, action_horizon=2)
            pol.fused_guide = fused
            diff.use_graph = fused
            assert pol.guide_route({0: None})[0] == ("library" if fused else "autograd")
            counts = {}
            saved = _count_calls(eng, counts)
            try:
                one = pol.get_action(obs[0])
                many = pol.get_actions(obs)
            finally:
                for k in saved:
                    delattr(eng, k)
            assert (counts == {"guided_loop": 2}) if fused else ("guided_loop" not in counts and counts["denoise_step"] == 40)
            got[fused] = (one, many)
        assert max_abs(got[True][0], got[False][0]) <= TOL_LOOP and max_abs(got[True][1], got[False][1]) <= TOL_LOOP
    finally:
        diff.sampler_rng, diff.seed, diff.use_graph = keep
