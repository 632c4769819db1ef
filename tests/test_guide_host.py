"""The library guide's host side (``dad_guide_grad`` / ``dad_guided_loop`` / ``dad_debug_guide_plan``): no device.

* the three entry points are exported and typed;
* every refusal returns its code and a message before anything touches a device (there is none here);
* ``plan_guide`` over in_dim x widths x layers x activation x rows: the grid covers the rows once, a plan that is not
  refused fits one CU's LDS, a refusal occurs exactly when a stated limit says so, the report decodes by name; the same
  sweep as a stand-alone program under ASan + UBSan (tests/sanitize/guide_check.cpp);
* ``GuideState.compile`` recognises the supported modules and says why it refuses the others;
* the routes of ``ValueGuidedPolicy.fused_guide`` against a recording engine that knows the new keywords.
"""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn as nn

from dynamics_aware_diffusion_amd import _engine
from tests import sampling_routes as routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAD_E_INVALID, DAD_E_STATE = -1, -2
LDS_BYTES = 160 * 1024          # dad::kLdsBytes (csrc/conv_shapes.hpp): one gfx950 CU
MAX_WIDTH, MIN_LAYERS, MAX_LAYERS = 512, 2, 4      # GM_* of csrc/conv_shapes.hpp, as the issue states them
ENTRY_POINTS = ("dad_guide_grad", "dad_guided_loop", "dad_debug_guide_plan")


def test_symbols_are_exported_and_typed():
    lib = _engine.load_library()
    for name in ENTRY_POINTS:
        assert name in _engine.ABI, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == _engine.ABI[name][1]
    assert len(_engine.ABI["dad_guide_grad"][1]) == 8 and len(_engine.ABI["dad_guided_loop"][1]) == 18
    # the guided loop is dad_sampler_loop with the guide and its weight after the condition
    base = list(_engine.ABI["dad_sampler_loop"][1])
    assert _engine.ABI["dad_guided_loop"][1] == base[:10] + [C.POINTER(_engine.DadGuideArgs), C.c_float] + base[10:]
    assert _engine._names("DAD_GD_ACTS") == ("tanh", "relu", "mish")
    assert _engine._names("DAD_GD_REFUSALS") == ("ok", "layers", "width", "activation", "in_dim", "last_width", "lds")
    assert C.sizeof(_engine.DadGuideArgs) == 4 * 11 + 4 + 8 * 12 + 8 + 8


def _args(in_dim=4, widths=(16, 1), act=0, null=None, padded=None, grad=0x1000, grad_bytes=1 << 30):
    """dad_guide_args whose pointers are non-null but point nowhere: every refusal comes before they are read."""
    a = _engine.DadGuideArgs()
    a.n_layers, a.in_dim, a.activation = len(widths), in_dim, act
    pads = [(in_dim + 31) // 32 * 32] + [(w + 31) // 32 * 32 for w in widths[:-1]]
    for i, w in enumerate(widths[:4]):
        a.widths[i] = w
    for i, w in enumerate((padded or pads)[:4]):
        a.padded[i] = w
    for i in range(min(len(widths), 4)):
        a.w_fwd[i], a.w_bwd[i], a.bias[i] = 0x1000, 0x1000, 0x1000
    if null is not None:
        getattr(a, null[0])[null[1]] = None
    a.grad, a.grad_bytes = grad, grad_bytes
    return a


def _refused(rc, code, *words):
    msg = _engine.load_library().dad_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg and all(w in msg for w in words), msg


def test_guide_grad_refuses_before_the_device():
    lib = _engine.load_library()

    def call(a=None, x=0x1000, g=0x1000, batch=3, horizon=8, td=6, null_args=False):
        a = _args() if a is None else a
        return lib.dad_guide_grad(None if null_args else C.byref(a), x, g, None, batch, horizon, td, None)

    _refused(call(null_args=True), DAD_E_INVALID, "missing")
    _refused(call(x=None), DAD_E_INVALID, "null")
    _refused(call(g=None), DAD_E_INVALID, "null")
    for batch, horizon, td in ((0, 8, 6), (-1, 8, 6), (3, 0, 6), (3, 8, 0)):
        _refused(call(batch=batch, horizon=horizon, td=td), DAD_E_INVALID, "positive")
    _refused(call(batch=1 << 20, horizon=1 << 10, td=8), DAD_E_INVALID, "2^31")
    _refused(call(a=_args(widths=(1,))), DAD_E_INVALID, "2 to 4")
    _refused(call(a=_args(widths=(8, 8, 8, 8, 1))), DAD_E_INVALID, "2 to 4")
    _refused(call(a=_args(widths=(513, 1))), DAD_E_INVALID, "512")
    _refused(call(a=_args(widths=(0, 1))), DAD_E_INVALID, "512")
    for act in (-1, 3):
        _refused(call(a=_args(act=act)), DAD_E_INVALID, "activation")
    _refused(call(a=_args(in_dim=7)), DAD_E_INVALID, "in_dim", "transition_dim")
    _refused(call(a=_args(in_dim=0)), DAD_E_INVALID, "in_dim")
    _refused(call(a=_args(widths=(16, 2))), DAD_E_INVALID, "one output")
    _refused(call(a=_args(in_dim=39, widths=(512, 512, 1), act=2), td=67), DAD_E_INVALID, "LDS")
    _refused(call(a=_args(padded=[32, 16])), DAD_E_INVALID, "padded[1]=16", "32")
    for field, layer in (("w_fwd", 0), ("w_fwd", 1), ("bias", 0), ("bias", 1), ("w_bwd", 0)):
        _refused(call(a=_args(null=(field, layer))), DAD_E_INVALID, "layer", "null")


def test_guided_loop_refuses_before_the_device():
    """On a created, unfinalised model: the arguments of the loop itself are refused first, then the model's state —
    and a guide is only looked at by a loop that would run."""
    from tests import forward_census as census
    lib = _engine.load_library()
    eng = census.host_engine(6, 32, (1, 2, 4), 32, 5, "fp32")
    a = _args()

    def call(m=eng._h, x=0x1000, steps=None, n_steps=4, batch=3, guide=a, gw=0.5, ws=0x1000, ws_bytes=1 << 30):
        return lib.dad_guided_loop(m, x, steps, n_steps, batch, None, 1, 0, None, 0, None if guide is None else C.byref(guide),
                                   gw, None, None, 0, ws, ws_bytes, None)

    _refused(call(m=None), DAD_E_INVALID, "null model")
    for n in (0, -2):
        _refused(call(n_steps=n), DAD_E_INVALID, "n_steps")
    bad = _engine.pack_sampler_steps({"tau": [3], **{k: [float("nan")] for k in _engine.SAMPLER_COEF_FIELDS}})
    _refused(call(steps=bad.ctypes.data, n_steps=1), DAD_E_INVALID, "step 0")
    _refused(call(), DAD_E_STATE)                      # not finalised: the same refusal with and without a guide
    _refused(call(guide=None), DAD_E_STATE)


def test_plan_refuses_bad_shapes():
    lib = _engine.load_library()
    out = (C.c_int32 * _engine._fields("DAD_GD_INTS")[1])()
    w = (C.c_int32 * 2)(16, 1)
    _refused(lib.dad_debug_guide_plan(4, w, 2, 0, 3, 8, 6, None), DAD_E_INVALID, "null")
    _refused(lib.dad_debug_guide_plan(4, None, 2, 0, 3, 8, 6, out), DAD_E_INVALID, "null")
    for batch, horizon, td in ((0, 8, 6), (3, -1, 6), (3, 8, 0)):
        _refused(lib.dad_debug_guide_plan(4, w, 2, 0, batch, horizon, td, out), DAD_E_INVALID, "positive")
    assert _engine.guide_plan(4, (16, 1), "gelu", 3, 8, 6)["refused"] == "activation"


SWEEP_IN = (1, 6, 39, 67)
SWEEP_W = (1, 16, 32, 33, 256, 512, 513)
SWEEP_ROWS = ((1, 8), (4, 8), (3, 11), (256, 32))          # B * H = 8, 32, 33, 8192


def _expected(in_dim, widths, act, td):
    """(refusal, LDS bytes) by the limits as stated, independently of the planner."""
    if not MIN_LAYERS <= len(widths) <= MAX_LAYERS:
        return "layers", 0
    if any(w < 1 or w > MAX_WIDTH for w in widths):
        return "width", 0
    if in_dim < 1 or in_dim > td:
        return "in_dim", 0
    if widths[-1] != 1:
        return "last_width", 0
    pad = lambda w: (w + 31) // 32 * 32
    lds = 33 * 4 * (pad(in_dim) + sum(pad(w) for w in widths[:-1]) * (2 if act == "mish" else 1))
    return ("lds" if lds > LDS_BYTES else None), lds


@pytest.mark.parametrize("in_dim", SWEEP_IN)
def test_plan_sweep(in_dim):
    nets = [(a, 1) for a in SWEEP_W] + [(a, b, 1) for a in SWEEP_W for b in SWEEP_W]
    nets += [(a, b, c, 1) for a in SWEEP_W for b in (1, 33, 512, 513) for c in (16, 512)]
    nets += [(16,), (16, 16), (16, 16, 16, 16, 1)]
    seen = set()
    for widths, act, (B, H) in itertools.product(nets, ("tanh", "relu", "mish"), SWEEP_ROWS):
        td = in_dim + (2 if len(widths) % 2 else 0)
        q = _engine.guide_plan(in_dim, widths, act, B, H, td)
        assert set(q) == {"layers", "padded", "rows_per_block", "threads", "grid", "lds_bytes", "refused"}
        want, lds = _expected(in_dim, widths, act, td)
        assert q["refused"] == want, (in_dim, widths, act, q)
        seen.add(want)
        assert q["rows_per_block"] == 32 and q["threads"] == 256 and q["layers"] == len(widths)
        assert q["grid"] * 32 >= B * H > (q["grid"] - 1) * 32          # every row in exactly one block
        if want is None:
            assert q["lds_bytes"] == lds <= LDS_BYTES
            assert q["padded"] == [(w + 31) // 32 * 32 for w in (in_dim,) + tuple(widths[:-1])]
        elif want == "lds":
            assert q["lds_bytes"] == lds > LDS_BYTES
    assert seen >= {None, "layers", "width", "last_width", "lds"}
    assert _engine.guide_plan(in_dim, (16, 1), "relu", 3, 8, in_dim - 1 or 1)["refused"] == ("in_dim" if in_dim > 1 else None)


def test_report_layout_is_registered_and_decodes():
    layouts = _engine.report_layouts()
    assert {"DAD_GD_INTS", "DAD_GD_ACTS", "DAD_GD_REFUSALS"} <= set(layouts)
    fields, length = _engine._fields("DAD_GD_INTS")
    assert length == len(fields) == 10 and all(span == 1 for _, _, span in fields)
    assert [name for name, _, _ in fields] == ["layers", "padded_in", "padded_1", "padded_2", "padded_3", "rows_per_block",
                                               "threads", "gx", "lds_bytes", "refused"]
    assert all(c.startswith("DAD_GD_") for k in ("DAD_GD_INTS", "DAD_GD_ACTS", "DAD_GD_REFUSALS") for c, _, _ in layouts[k])


def test_guide_host_logic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "guide_check"
    src = os.path.join(ROOT, "tests", "sanitize", "guide_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "guide host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# ------------------------------------------------------------------------------------------------ GuideState.compile
def _seq(*widths, act=nn.Tanh, in_dim=6, bias=True):
    mods, k = [], in_dim
    for i, n in enumerate(widths):
        mods.append(nn.Linear(k, n, bias=bias))
        if i + 1 < len(widths):
            mods.append(act())
        k = n
    return nn.Sequential(*mods)


def test_compile_recognises_the_supported_modules():
    for act, name in ((nn.Tanh, "tanh"), (nn.ReLU, "relu"), (nn.Mish, "mish")):
        for widths in ((16, 1), (33, 7, 1), (64, 64, 64, 1)):
            state, why = _engine.GuideState.compile(_seq(*widths, act=act), 6, host=True)
            assert state is not None and why is None, why
            assert state.activation == name and state.widths == list(widths) and state.in_dim == 6
            assert state.padded == [32] + [(w + 31) // 32 * 32 for w in widths[:-1]]
            assert state.args.n_layers == len(widths) and list(state.args.padded)[:len(widths)] == state.padded
            assert state.plan(3, 11, 8) == _engine.guide_plan(6, widths, name, 3, 11, 8)
    state, why = _engine.GuideState.compile(_seq(16, 1, bias=False), 6, host=True)
    assert state is not None, why
    with pytest.raises(TypeError):
        _engine.GuideState()


def test_compile_refuses_with_a_reason():
    def refused(module, *words, in_dim=6):
        state, why = _engine.GuideState.compile(module, in_dim, host=True)
        assert state is None and all(w in why for w in words), why

    class Free(nn.Module):
        def forward(self, obs):
            return obs.sum(-1, keepdim=True)

    refused(Free(), "Free", "nn.Sequential")
    refused(nn.Sequential(nn.Linear(6, 1)), "no hidden layer")
    refused(nn.Sequential(nn.Linear(6, 16), nn.Tanh()), "alternate")
    refused(nn.Sequential(nn.Linear(6, 16), nn.Linear(16, 4), nn.Linear(4, 1)), "activations are Linear")
    refused(nn.Sequential(nn.Linear(6, 16), nn.GELU(), nn.Linear(16, 1)), "GELU")
    refused(nn.Sequential(nn.Linear(6, 16), nn.Tanh(), nn.Linear(16, 16), nn.ReLU(), nn.Linear(16, 1)), "ReLU", "Tanh")
    refused(_seq(16, 1), "reads 6", "given 4", in_dim=4)
    refused(nn.Sequential(nn.Linear(6, 16), nn.Tanh(), nn.Linear(8, 1)), "chain")
    refused(_seq(16, 2), "2 outputs")
    refused(_seq(16, 1).double(), "float64")
    refused(_seq(513, 1), "planner", "width")
    refused(_seq(8, 8, 8, 8, 1), "planner", "layers")
    refused(_seq(512, 512, 1, act=nn.Mish, in_dim=39), "planner", "lds", in_dim=39)


# ------------------------------------------------------------------------------------------------ routes
class GuideRecordingEngine(routes.RecordingEngine):
    """The recording stub with the two keywords a library guide adds to the fused loops."""

    def _guided(self, name, guide, guide_weight):
        self.events.append(f"{name} guide={type(guide).__name__} in{guide.in_dim} w{guide_weight:g}")

    def sample_loop(self, x, n_steps, *, guide=None, guide_weight=0.0, **kw):
        if guide is not None:
            self._guided("guided", guide, guide_weight)
        super().sample_loop(x, n_steps, **kw)

    def sampler_loop(self, x, steps, *, guide=None, guide_weight=0.0, **kw):
        if guide is not None:
            self._guided("guided", guide, guide_weight)
        super().sampler_loop(x, steps, **kw)


def _policy(events, fused, sampler="ddpm", rng="philox", graph=False):
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet, ValueGuidedPolicy
    diff = GaussianDiffusion(TemporalUnet(routes.TD, dim=32, dim_mults=(1, 2)), routes.HORIZON, routes.OBS, routes.ACT,
                             n_timesteps=routes.T_TRAINED)
    eng = GuideRecordingEngine(events)
    diff._engine = lambda device: eng
    diff.sampler_rng, diff.seed, diff.use_graph = rng, routes.SEED, graph
    if sampler == "ddpm":
        diff.n_timesteps = 4
    else:
        diff.set_sampler("ddim", steps=3, eta=0.5)
    pol = ValueGuidedPolicy(diff, None, _seq(16, 1, in_dim=routes.OBS), guide_weight=0.5)
    pol.fused_guide = fused
    return pol


@pytest.mark.parametrize("graph", (False, True))
@pytest.mark.parametrize("rng", ("philox", "torch"))
@pytest.mark.parametrize("sampler", ("ddpm", "ddim"))
def test_opt_in_with_cond0_only_is_one_fused_loop_carrying_the_guide(sampler, rng, graph):
    events = []
    pol = _policy(events, True, sampler, rng, graph)
    cond = {0: routes._ramp((routes.B, routes.TD), 6)}
    assert pol.guide_route(cond, routes.B)[0] == "library"
    torch.manual_seed(1234)
    out = pol.sample_loop(batch_size=routes.B, conditions=cond, row_offset=routes.ROW_OFFSET)
    assert out.shape == (routes.B, routes.HORIZON, routes.TD)
    calls = [e for e in events if not e.startswith("fill")]
    assert len(calls) == 2 and calls[0] == f"guided guide=GuideState in{routes.OBS} w0.5", calls
    assert calls[1].startswith("loop n4 " if sampler == "ddpm" else "sloop k") and calls[1].endswith(f"G{int(graph)}"), calls


def test_opt_in_with_a_condition_at_step_2_takes_the_stepwise_route():
    events = []
    pol = _policy(events, True)
    cond = {0: routes._ramp((routes.B, routes.TD), 6), 2: routes._ramp((routes.B, routes.TD), 7)}
    route, why = pol.guide_route(cond, routes.B)
    assert route == "autograd" and "beyond horizon step 0" in why
    pol.sample_loop(batch_size=routes.B, conditions=cond, row_offset=routes.ROW_OFFSET)
    calls = [e for e in events if not e.startswith("fill")]
    assert len(calls) == 4 and all(c.startswith("step t") and " g-" not in c and c.endswith("w0.5") for c in calls), calls


def test_routes_say_why():
    from dynamics_aware_diffusion_amd import GuidedPolicy
    pol = _policy([], False)
    assert pol.guide_route() == ("autograd", "fused_guide is off")
    assert GuidedPolicy.fused_guide is False
    pol.fused_guide = True
    assert pol.guide_route()[0] == "library"
    pol.guide_weight = 0.0
    assert pol.guide_route()[0] == "unguided"
    pol.guide_weight = 0.5
    pol.value_model = nn.Sequential(nn.Linear(routes.OBS, 16), nn.GELU(), nn.Linear(16, 1))
    route, why = pol.guide_route()
    assert route == "autograd" and "GELU" in why
    plain = GuidedPolicy(pol.diffusion, None, guide_fn=routes._guide, guide_weight=0.5)
    plain.fused_guide = True
    assert plain.guide_route() == ("autograd", "only ValueGuidedPolicy's guide has a library form")


def test_opt_out_makes_the_calls_it_always_made():
    """fused_guide off: the guided loop is one engine step per iteration with an autograd gradient, on the plain
    recording engine, which knows no guide keyword (the traces themselves: test_sampling_routes_host.py)."""
    events = []
    pol = _policy(events, False)
    pol.diffusion._engine = (lambda eng: lambda device: eng)(routes.RecordingEngine(events))
    pol.sample_loop(batch_size=routes.B, conditions={0: routes._ramp((routes.B, routes.TD), 6)})
    calls = [e for e in events if not e.startswith("fill")]
    assert len(calls) == 4 and all(c.startswith("step t") and " g-" not in c for c in calls), calls
