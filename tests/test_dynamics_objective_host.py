"""The dynamics-aware objective's host side (``dad_train_dynamics_objective_*``, ``losses.DynamicsAwareLoss``): no device.

* the three entry points and the plan report are exported and typed;
* every refusal returns its code and a message before anything touches a device (there is none here);
* the plan over batch x horizon x (state, action) widths x form: the launches, the workspace sizes, and the form, grids
  and LDS sizes of ``dad_debug_violation_grad_plan`` for the same shape;
* the report section has the field names listed here;
* ``DynamicsAwareLoss`` raises its constructor errors and ``route()`` gives its answers on an engine without a device;
* tests/sanitize/dynamics_objective_check.cpp (the host planner only) under the address / UB sanitizers, as a program.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from dynamics_aware_diffusion_amd import _engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAD_E_INVALID, DAD_E_STATE, DAD_E_WORKSPACE = -1, -2, -6
LDS_BYTES = 160 * 1024
ENTRY_POINTS = ("dad_train_dynamics_objective_workspace_bytes", "dad_train_dynamics_objective_forward",
                "dad_train_dynamics_objective_backward", "dad_debug_dynamics_objective_plan")


def _engine_for(n, m, H, real_H=None):
    mults = (1, 2) if H % 8 else (1, 2, 4)
    return _engine.HipEngine(transition_dim=n + m, dim=32, channels=tuple(32 * k for k in mults), horizon=H, n_timesteps=20,
                             training=True)


def _args(n=4, od=4, m=2, null=None):
    a = _engine.DadProjectArgs()
    for k in ("P", "obs_mean", "obs_std", "act_mean", "act_std"):
        setattr(a, k, None if k == null else 0x1000)
    a.state_dim, a.observation_dim, a.action_dim = n, od, m
    return a


def _refused(rc, code, *words):
    msg = _engine.load_library().dad_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg and all(w in msg for w in words), msg


def test_symbols_are_exported_and_typed():
    lib = _engine.load_library()
    for name in ENTRY_POINTS:
        assert name in _engine.ABI, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == _engine.ABI[name][1]
    # the arguments of the existing pair plus: projection, P's side, form, two weights, timestep weights (and parts for loss)
    assert len(_engine.ABI["dad_train_dynamics_objective_forward"][1]) == len(_engine.ABI["dad_train_objective_forward"][1]) + 6
    assert len(_engine.ABI["dad_train_dynamics_objective_backward"][1]) == len(_engine.ABI["dad_train_objective_backward"][1]) + 6


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_every_refusal_comes_before_the_device(entry):
    lib = _engine.load_library()
    p, big, B, D = 0x1000, 1 << 30, 3, 196
    one = (C.c_void_p * 1)(p)

    def call(h, a=None, null_args=False, x0=p, aux=p, loss_type=2, p_dim=D, form=-1, batch=B, saved=p):
        a = _args() if a is None else a
        pa = None if null_args else C.byref(a)
        if entry == "fwd":      # aux: the parts
            return lib.dad_train_dynamics_objective_forward(h, x0, p, p, None, loss_type, pa, p_dim, form, 1.0, 0.1, None, aux, batch,
                                                            saved, big, None)
        return lib.dad_train_dynamics_objective_backward(h, x0, p, None, loss_type, pa, p_dim, form, 1.0, 0.1, None, aux, one, 1, one, 1,
                                                         batch, saved, big, p, big, None)

    eng = _engine_for(4, 2, 32)
    h = eng._h
    _refused(call(None), DAD_E_INVALID, "null model")
    for kw in ({"x0": None}, {"aux": None}, {"saved": None}):
        _refused(call(h, **kw), DAD_E_INVALID, "null pointer")
    for lt in (0, 3):
        _refused(call(h, loss_type=lt), DAD_E_INVALID, "loss_type")
    for batch in (0, -2):
        _refused(call(h, batch=batch), DAD_E_INVALID, "batch must be positive")
    _refused(call(h, null_args=True), DAD_E_INVALID, "projection arguments missing")
    for k in ("P", "obs_mean", "obs_std", "act_mean", "act_std"):
        _refused(call(h, a=_args(null=k)), DAD_E_INVALID, "projection arguments missing")
    _refused(call(h, a=_args(n=6, od=4)), DAD_E_INVALID, "state_dim=6", "observation_dim=4")
    _refused(call(h, a=_args(m=3)), DAD_E_INVALID, "transition_dim=6")
    for form in (-2, 2):
        _refused(call(h, form=form), DAD_E_INVALID, f"form={form}")
    for p_dim in (195, 52, 0):          # P not (D, D) for this horizon
        _refused(call(h, p_dim=p_dim), DAD_E_INVALID, f"({p_dim}, {p_dim})", "(196, 196)", "horizon 32")
    # everything about the arguments is in order: what is left is the state of the model (never finalized here)
    _refused(call(h), DAD_E_STATE, "finalize")
    # a forced row form beyond one CU's LDS: n = 39, m = 28, H = 40: D = 2719, 17 D 4 bytes = 184 892 > 163 840
    wide = _engine_for(39, 28, 40)
    _refused(call(wide._h, a=_args(39, 39, 28), p_dim=2719, form=0), DAD_E_INVALID, "row form", "D=2719")
    _refused(call(wide._h, a=_args(39, 39, 28), p_dim=2719, form=-1), DAD_E_STATE, "finalize")
    # training not enabled
    plain = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20)
    _refused(call(plain._h), DAD_E_INVALID, "training mode is off")


def test_workspace_query_and_plan_refuse_bad_shapes():
    lib = _engine.load_library()
    eng = _engine_for(4, 2, 32)
    sv, sc, a = C.c_size_t(), C.c_size_t(), _args()
    _refused(lib.dad_train_dynamics_objective_workspace_bytes(None, C.byref(a), -1, 3, C.byref(sv), C.byref(sc)), DAD_E_INVALID, "null")
    _refused(lib.dad_train_dynamics_objective_workspace_bytes(eng._h, None, -1, 3, C.byref(sv), C.byref(sc)), DAD_E_INVALID, "null")
    _refused(lib.dad_train_dynamics_objective_workspace_bytes(eng._h, C.byref(a), -1, 0, C.byref(sv), C.byref(sc)), DAD_E_INVALID, "positive")
    _refused(lib.dad_train_dynamics_objective_workspace_bytes(eng._h, C.byref(a), 5, 3, C.byref(sv), C.byref(sc)), DAD_E_INVALID, "form=5")
    for kw, word in (({"batch": 0}, "positive"), ({"state_dim": 6}, "state_dim=6"), ({"action_dim": 1}, "transition_dim=6")):
        args = dict(batch=3, state_dim=4, observation_dim=4, action_dim=2)
        args.update(kw)
        with pytest.raises(_engine.DadError, match=word):
            eng.dynamics_objective_plan(**args)
    with pytest.raises(ValueError, match="form"):
        eng.dynamics_objective_plan(3, 4, 4, 2, "mfma")
    plain = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20)
    with pytest.raises(_engine.DadError, match="dad_model_set_training"):
        plain.dynamics_objective_plan(3, 4, 4, 2)


SWEEP_B = (1, 3, 32, 33, 256)
SWEEP_H = (8, 24, 32)
SWEEP_NM = ((4, 2), (17, 6), (39, 28))


@pytest.mark.parametrize("n,m", SWEEP_NM)
@pytest.mark.parametrize("H", SWEEP_H)
def test_plan_sweep(H, n, m):
    lib = _engine.load_library()
    eng = _engine_for(n, m, H)
    st = _engine.ProjectionState.host(n, n, m)
    D, td = (H + 1) * n + H * m, n + m
    al = lambda floats: (floats + 63) // 64 * 64          # noqa: E731
    for B in SWEEP_B:
        sv0, sc0 = eng._objective_bytes(B)
        assert eng.objective_plan(B)["launches"] and len(eng.objective_plan(B)["launches"]) == 9
        for form in (None, "row", "gemm"):
            vg = st.grad_plan(B, H, form)
            q = eng.dynamics_objective_plan(B, state=st, form=form)
            assert q == eng.dynamics_objective_plan(B, n, n, m, form)
            # the form and the launches' geometry are the violation pair's for x0_hat's shape
            assert q["form"] == vg["form"] and q["refused"] == vg["refused"] and q["D"] == D and q["horizon"] == H
            gemm = q["form"] == "gemm"
            if form is None:
                assert gemm == (17 * D * 4 > LDS_BYTES or (D >= 512 and B >= 32)) and not q["refused"]
            kinds = [l["kind"] for l in q["launches"]]
            assert kinds == (["fwd_gemm", "fwd_parts", "bwd_gemm", "bwd_scatter"] if gemm else ["fwd_row", "fwd_parts", "bwd_row"])
            assert q["fwd_launches"] == 2 and q["objective_launches"] == 9
            fwd, parts, bwd = q["launches"][:3]
            assert fwd["grid"] == vg["fwd"]["grid"] and fwd["lds_bytes"] == vg["fwd"]["lds_bytes"]
            assert fwd["rows_per_block"] == vg["fwd"]["rows_per_block"]
            assert bwd["grid"] == vg["bwd"]["grid"] and bwd["lds_bytes"] == vg["bwd"]["lds_bytes"]
            assert bwd["rows_per_block"] == vg["bwd"]["rows_per_block"]
            assert parts["grid"] == (1, 1) and parts["threads"] == 256 and parts["lds_bytes"] == 0
            assert fwd["threads"] == (256 if gemm else 1024) and bwd["threads"] == (256 if gemm else 1024)
            if gemm:
                scatter = q["launches"][3]
                assert scatter["grid"] == (vg["bwd"]["scatter_gx"], 1) and scatter["threads"] == 256
                assert q["col_blocks"] == fwd["grid"][1] == -(-D // 32)
            else:
                assert q["col_blocks"] == 0
            if not q["refused"]:
                assert all(l["lds_bytes"] <= LDS_BYTES for l in q["launches"])
            # the workspaces: the fused objective's, rounded up to 256 bytes, then r | partial sums or violation; g
            assert q["saved_base"] == -(-sv0 // 256) * 256 and q["scratch_base"] == -(-sc0 // 256) * 256
            saved_floats = al(B * D) + (al(B * q["col_blocks"]) if gemm else al(B))
            scratch_floats = al(B * D) if gemm else 0
            assert q["saved_bytes"] == q["saved_base"] + 4 * saved_floats
            assert q["scratch_bytes"] == q["scratch_base"] + 4 * scratch_floats
            assert q["r_offset"] == 0 and (q["part_offset"] if gemm else q["violation_offset"]) == al(B * D) and q["g_offset"] == 0
            sv, sc = C.c_size_t(), C.c_size_t()
            assert lib.dad_train_dynamics_objective_workspace_bytes(eng._h, C.byref(st.args), _engine.VIOLATION_FORMS[form], B,
                                                                    C.byref(sv), C.byref(sc)) == 0
            assert (sv.value, sc.value) == (q["saved_bytes"], q["scratch_bytes"])
            assert eng._objective_bytes(B) == (sv0, sc0)


def test_zero_padded_horizon_plans_for_the_real_one():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    diff = GaussianDiffusion(TemporalUnet(6, dim=32, dim_mults=(1, 2, 4)), 24, 4, 2, n_timesteps=20)
    from dynamics_aware_diffusion_amd.losses import DynamicsAwareLoss
    loss = DynamicsAwareLoss.host(diff, 4, 2, 4, 24)
    eng = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=24, n_timesteps=20, training=True)
    q = eng.dynamics_objective_plan(3, 4, 4, 2)
    assert q["horizon"] == 24 and q["D"] == 25 * 4 + 24 * 2 == loss._D


def test_report_layout_is_registered_and_decodes():
    layouts = _engine.report_layouts()
    assert {"DAD_DO_HEADER", "DAD_DO_REC_INTS", "DAD_DO_KINDS"} <= set(layouts)
    assert _engine._names("DAD_DO_HEADER") == (
        "form", "D", "horizon", "col_blocks", "refused", "saved_base", "saved_bytes", "scratch_base", "scratch_bytes", "r_offset",
        "part_offset", "violation_offset", "g_offset", "objective_launches", "fwd_launches", "record_ints", "launches")
    assert _engine._names("DAD_DO_REC_INTS") == ("kind", "gx", "gy", "threads", "lds_bytes", "rows_per_block")
    assert _engine._names("DAD_DO_KINDS") == ("fwd_row", "fwd_gemm", "fwd_parts", "bwd_row", "bwd_gemm", "bwd_scatter")
    for section in ("DAD_DO_HEADER", "DAD_DO_REC_INTS", "DAD_DO_KINDS"):
        assert all(c.startswith("DAD_DO_") and span == 1 for c, _, span in layouts[section])
    eng = _engine_for(4, 2, 32)
    ints = _engine._fetch(eng.lib.dad_debug_dynamics_objective_plan, eng._h, 4, 4, 4, 2, -1)
    head = _engine._decode("DAD_DO_HEADER", ints)
    assert head["record_ints"] == _engine._fields("DAD_DO_REC_INTS")[1]
    assert len(ints) == _engine._fields("DAD_DO_HEADER")[1] + head["launches"] * head["record_ints"]


def _diffusion(horizon=32, **kw):
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    return GaussianDiffusion(TemporalUnet(6, dim=32, dim_mults=(1, 2, 4)), horizon, 4, 2, n_timesteps=20, **kw)


def test_constructor_errors():
    from dynamics_aware_diffusion_amd.losses import DynamicsAwareLoss
    from tests.golden import cases
    diff, norm = _diffusion(), cases.NormalizerStub(4, 2)
    D = 33 * 4 + 32 * 2
    with pytest.raises(ValueError, match=r"projection matrix is \(195, 195\), expected \(196, 196\)"):
        DynamicsAwareLoss(diff, torch.zeros(195, 195), norm, 4, 2, 4, 32, device="cpu")
    with pytest.raises(ValueError, match=r"expected \(148, 148\)"):          # the projector of another horizon
        DynamicsAwareLoss(diff, torch.zeros(D, D), norm, 4, 2, 4, 24, device="cpu")
    with pytest.raises(ValueError, match=r"timestep_weights is \(19,\), expected \(20,\)"):
        DynamicsAwareLoss(diff, torch.zeros(D, D), norm, 4, 2, 4, 32, timestep_weights=torch.ones(19), device="cpu")
    with pytest.raises(RuntimeError, match="ROCm device"):                   # as ProjectionLoss: there is no CPU path
        DynamicsAwareLoss(diff, torch.zeros(D, D), norm, 4, 2, 4, 32, device="cpu")


def test_routes_say_why():
    import torch.nn as nn
    from dynamics_aware_diffusion_amd.losses import DynamicsAwareLoss
    diff = _diffusion()
    loss = DynamicsAwareLoss.host(diff, 4, 2, 4, 32)
    eng = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20, training=True)
    loss._plan_engine = lambda: eng
    assert diff.fused_objective is False
    assert loss.route(4) == ("default", "fused_objective is off")
    diff.fused_objective = True
    assert loss.route(4) == ("library", "one node, row form")
    loss.form = "gemm"
    assert loss.route(33) == ("library", "one node, gemm form")
    loss.form = None
    x0 = torch.zeros(4, 32, 6, requires_grad=True)
    with torch.enable_grad():
        assert loss.route(4, x0) == ("default", "x_0 requires grad")
    assert loss.route(4, x0)[0] == "library"                               # (under no_grad nothing is differentiated)
    assert loss.route(4, x0.detach())[0] == "library"
    for fn in (nn.SmoothL1Loss(reduction="none"), nn.MSELoss()):             # a replaced loss, a reduced one
        keep, diff.loss_fn = diff.loss_fn, fn
        route, why = loss.route(4)
        assert route == "default" and "plain L1 / L2" in why
        diff.loss_fn = keep
    route, why = loss.route(0)
    assert route == "default" and "planner" in why and "positive" in why
    # a model whose widths the projector does not fit
    other = _engine.HipEngine(transition_dim=8, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20, training=True)
    loss._plan_engine = lambda: other
    route, why = loss.route(4)
    assert route == "default" and "transition_dim=8" in why
    # a forced row form beyond a CU's LDS
    wide = DynamicsAwareLoss.host(diff, 39, 28, 39, 40)
    weng = _engine_for(39, 28, 40)
    wide._plan_engine = lambda: weng
    wide.form = "row"
    assert wide.route(4) == ("default", "planner: the forced row form exceeds one CU's LDS")
    wide.form = None
    assert wide.route(4) == ("library", "one node, gemm form")


def test_planner_under_address_and_ub_sanitizers(tmp_path):
    """tests/sanitize/dynamics_objective_check.cpp: a stand-alone program over the host planner (nothing is loaded into
    Python under a sanitizer), compiled host-only with -fsanitize=address,undefined."""
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "dynamics_objective_check"
    src = os.path.join(ROOT, "tests", "sanitize", "dynamics_objective_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "dynamics objective host logic ok" in run.stdout
