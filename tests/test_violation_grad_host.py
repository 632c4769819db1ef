"""The violation gradient's host side (``dad_projection_violation_fwd`` / ``_bwd``): no device.

* the four entry points are exported and typed;
* every refusal returns its code and a message before anything touches a device (there is none here);
* ``plan_violation_grad`` over D x batch x form: the planner's own choice is never refused, a forced row form exactly
  when a row and its 16 partial sets exceed one CU's LDS, the grids cover the batch and D, the workspace holds r, and
  the report decodes by name.
"""
import ctypes as C

import pytest

from dynamics_aware_diffusion_amd import _engine

DAD_E_INVALID, DAD_E_WORKSPACE = -1, -6
LDS_BYTES = 160 * 1024          # dad::kLdsBytes (csrc/conv_shapes.hpp): one gfx950 CU
ENTRY_POINTS = ("dad_violation_grad_workspace_bytes", "dad_projection_violation_fwd", "dad_projection_violation_bwd",
                "dad_debug_violation_grad_plan")
N, M = 4, 2                     # state and action widths of the sweep: D = (H + 1) N + H M = 6 H + 4


def _horizon(D):
    assert (D - N) % (N + M) == 0, D
    return (D - N) // (N + M)


def _args(n=N, od=N, m=M, null=None):
    """dad_project_args whose pointers are non-null but point nowhere: every refusal comes before they are read."""
    a = _engine.DadProjectArgs()
    for k in ("P", "obs_mean", "obs_std", "act_mean", "act_std"):
        setattr(a, k, None if k == null else 0x1000)
    a.state_dim, a.observation_dim, a.action_dim = n, od, m
    return a


def test_symbols_are_exported_and_typed():
    lib = _engine.load_library()
    for name in ENTRY_POINTS:
        assert name in _engine.ABI, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == _engine.ABI[name][1]
    assert len(_engine.ABI["dad_projection_violation_fwd"][1]) == len(_engine.ABI["dad_projection_violation_bwd"][1]) == 9
    assert _engine._names("DAD_VG_FORMS") == ("row", "gemm")
    assert _engine.VIOLATION_FORMS == {None: -1, "row": 0, "gemm": 1}


def _refused(rc, code, *words):
    msg = _engine.load_library().dad_last_error().decode()
    assert rc == code, (rc, msg)
    assert msg and all(w in msg for w in words), msg


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_every_refusal_comes_before_the_device(entry):
    lib = _engine.load_library()
    fn = lib.dad_projection_violation_fwd if entry == "fwd" else lib.dad_projection_violation_bwd
    H, B = 8, 3
    big = 1 << 30

    def call(a=None, p1=0x1000, p2=0x1000, ws=0x1000, ws_bytes=big, batch=B, horizon=H, form=-1, null_args=False):
        a = _args() if a is None else a
        return fn(None if null_args else C.byref(a), p1, p2, ws, ws_bytes, batch, horizon, form, None)

    _refused(call(null_args=True), DAD_E_INVALID, "missing")
    for k in ("P", "obs_mean", "obs_std", "act_mean", "act_std"):
        _refused(call(a=_args(null=k)), DAD_E_INVALID, "missing")
    _refused(call(p1=None), DAD_E_INVALID, "null")
    _refused(call(p2=None), DAD_E_INVALID, "null")
    _refused(call(ws=None), DAD_E_INVALID, "null workspace")
    for batch, horizon in ((0, H), (-1, H), (B, 0), (B, -3)):
        _refused(call(batch=batch, horizon=horizon), DAD_E_INVALID, "positive")
    _refused(call(a=_args(n=6, od=4)), DAD_E_INVALID, "state_dim=6", "observation_dim=4")
    for form in (-2, 2):
        _refused(call(form=form), DAD_E_INVALID, f"form={form}")
    # a forced row form whose row does not fit LDS: D = 2410 (H = 401), 17 D 4 bytes = 163 880 > 163 840
    _refused(call(horizon=_horizon(2410), form=0), DAD_E_INVALID, "row form", "D=2410")
    # a workspace one byte short (the same call with enough of it would go on to the device)
    need = C.c_size_t()
    a = _args()
    for form in (-1, 0, 1):
        assert lib.dad_violation_grad_workspace_bytes(C.byref(a), B, H, form, C.byref(need)) == 0
        assert need.value >= B * 52 * 4
        _refused(call(ws_bytes=need.value - 1, form=form), DAD_E_WORKSPACE, str(need.value))
    _refused(call(ws_bytes=0), DAD_E_WORKSPACE, "workspace")


def test_workspace_query_and_plan_refuse_bad_shapes():
    lib = _engine.load_library()
    need, a = C.c_size_t(), _args()
    out = (C.c_int32 * _engine._fields("DAD_VG_INTS")[1])()
    _refused(lib.dad_violation_grad_workspace_bytes(None, 3, 8, -1, C.byref(need)), DAD_E_INVALID, "null")
    _refused(lib.dad_violation_grad_workspace_bytes(C.byref(a), 3, 8, -1, None), DAD_E_INVALID, "null")
    _refused(lib.dad_violation_grad_workspace_bytes(C.byref(a), 0, 8, -1, C.byref(need)), DAD_E_INVALID, "positive")
    _refused(lib.dad_violation_grad_workspace_bytes(C.byref(a), 3, 8, 5, C.byref(need)), DAD_E_INVALID, "form=5")
    _refused(lib.dad_debug_violation_grad_plan(4, 4, 2, 3, 8, -1, None), DAD_E_INVALID, "null")
    _refused(lib.dad_debug_violation_grad_plan(6, 4, 2, 3, 8, -1, out), DAD_E_INVALID, "state_dim=6")
    _refused(lib.dad_debug_violation_grad_plan(4, 4, 2, 3, 0, -1, out), DAD_E_INVALID, "positive")
    _refused(lib.dad_debug_violation_grad_plan(4, 4, 2, 3, 8, 7, out), DAD_E_INVALID, "form=7")
    with pytest.raises(ValueError, match="form"):
        _engine.violation_grad_plan(4, 4, 2, 3, 8, "mfma")


SWEEP_D = (52, 196, 511, 512, 514, 2183, 2409, 2410, 4000)
SWEEP_B = (1, 31, 32, 33, 513)


def _dims(D):
    """(n, od, m, H) with D = (H + 1) n + H m: the 4 + 2 system where 6 divides D - 4, else one that fits."""
    if (D - N) % (N + M) == 0:
        return N, N, M, (D - N) // (N + M)
    for n, m in ((3, 1), (5, 2), (1, 1), (2, 1), (7, 3), (11, 1)):
        if D > n and (D - n) % (n + m) == 0:
            return n, n, m, (D - n) // (n + m)
    raise AssertionError(D)


@pytest.mark.parametrize("D", SWEEP_D)
def test_plan_sweep(D):
    n, od, m, H = _dims(D)
    assert (H + 1) * n + H * m == D
    row_lds = 17 * D * 4                                   # a row + its 16 partial sets (project_row_lds_bytes)
    st = _engine.ProjectionState.host(n, od, m)
    for B in SWEEP_B:
        for form in (None, "row", "gemm"):
            q = st.grad_plan(B, H, form)
            assert q == _engine.violation_grad_plan(n, od, m, B, H, form)
            assert set(q) == {"form", "refused", "workspace_bytes", "fwd", "bwd"}
            assert set(q["fwd"]) == {"rows_per_block", "grid", "lds_bytes", "sum_gx"}
            assert set(q["bwd"]) == {"rows_per_block", "grid", "lds_bytes", "scatter_gx"}
            if form is None:
                assert not q["refused"], (D, B)
                # the rule: the GEMM form from D = 512 at batches of 32+, and wherever a row does not fit LDS
                assert q["form"] == ("gemm" if row_lds > LDS_BYTES or (D >= 512 and B >= 32) else "row"), (D, B)
            else:
                assert q["form"] == form
                assert q["refused"] == (form == "row" and row_lds > LDS_BYTES), (D, B, form)
            assert q["workspace_bytes"] >= B * D * 4
            need = C.c_size_t()
            assert _engine.load_library().dad_violation_grad_workspace_bytes(
                C.byref(st.args), B, H, _engine.VIOLATION_FORMS[form], C.byref(need)) == 0
            assert need.value == q["workspace_bytes"] and need.value % 256 == 0
            for side in ("fwd", "bwd"):
                p = q[side]
                gx, gy = p["grid"]
                assert gx >= 1 and gy >= 1 and gx * p["rows_per_block"] >= B > (gx - 1) * p["rows_per_block"]
                if q["form"] == "gemm":
                    assert p["rows_per_block"] == 32 and gy * 32 >= D > (gy - 1) * 32
                    assert p["lds_bytes"] <= LDS_BYTES
                else:
                    assert gy == 1 and p["rows_per_block"] in (1, 4)
                    assert (p["lds_bytes"] > LDS_BYTES) == (side == "fwd" and q["refused"])
            if q["form"] == "gemm":
                assert q["fwd"]["sum_gx"] * 256 >= B
                assert q["bwd"]["scatter_gx"] * 256 >= B * H * (od + m) > (q["bwd"]["scatter_gx"] - 1) * 256
                assert q["workspace_bytes"] >= (2 * B * D + B * q["fwd"]["grid"][1]) * 4
            else:
                assert q["fwd"]["sum_gx"] == 0 and q["bwd"]["scatter_gx"] == 0
                assert q["fwd"]["lds_bytes"] == q["fwd"]["rows_per_block"] * row_lds and q["bwd"]["lds_bytes"] == 2 * D * 4
                # the forward is the launch dad_projection_violation makes: same kernel, same grid, same bits
                pp, p_fwd = st.plan(B, H, violation=True), q["fwd"]
                assert pp["rows_per_block"] == p_fwd["rows_per_block"] and pp["grid"] == p_fwd["grid"]
                assert pp["lds_bytes"] == p_fwd["lds_bytes"] and pp["refused"] == q["refused"]


def test_report_layout_is_registered_and_decodes():
    layouts = _engine.report_layouts()
    assert "DAD_VG_INTS" in layouts and "DAD_VG_FORMS" in layouts
    fields, length = _engine._fields("DAD_VG_INTS")
    assert length == len(fields) == 13 and all(span == 1 for _, _, span in fields)
    assert [name for name, _, _ in fields] == [
        "form", "fwd_rows_per_block", "fwd_gx", "fwd_gy", "fwd_lds_bytes", "fwd_sum_gx", "bwd_rows_per_block", "bwd_gx",
        "bwd_gy", "bwd_lds_bytes", "bwd_scatter_gx", "workspace_bytes", "refused"]
    assert all(c.startswith("DAD_VG_") for c, _, _ in layouts["DAD_VG_INTS"] + layouts["DAD_VG_FORMS"])
