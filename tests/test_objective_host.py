"""CPU tests (`-m "not gpu"`) of the fused training objective's host side: the new entry points of include/dad.h are
exported and refuse bad arguments with DAD_E_INVALID and a message before anything touches a device, the time-MLP
gradient list is a list of its own (dad_train_grad_info is unchanged), the workspace query adds to the existing sizes,
and the workspace layout satisfies the kernels' assumptions (tests/sanitize/objective_check.cpp under the address / UB
sanitizers)."""
import ctypes as C
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = -1

NEW_SYMBOLS = ("dad_model_load_train_schedule", "dad_train_time_grad_count", "dad_train_time_grad_info",
               "dad_train_objective_workspace_bytes", "dad_train_objective_forward", "dad_train_objective_backward",
               "dad_debug_objective_offsets", "dad_debug_objective_plan")


def _model(lib, training=True, td=6, dim=32, mults=(1, 2, 4), horizon=32):
    from tests.test_long_horizon_host import _cfg
    h = C.c_void_p()
    assert lib.dad_model_create(C.byref(_cfg(td, dim, mults, horizon)), C.byref(h)) == 0, lib.dad_last_error()
    if training:
        assert lib.dad_model_set_training(h, 1) == 0, lib.dad_last_error()
    return h


def test_new_symbols_are_exported_and_typed():
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    for name in NEW_SYMBOLS:
        assert name in _engine.ABI, name
        assert getattr(lib, name).argtypes is not None
    assert _engine.LOSS_TYPES == {"l1": 1, "l2": 2}


def test_time_gradient_list_is_a_list_of_its_own():
    """time_mlp.1 / .3, then every block's time_mlp.1 in launch order; dad_train_grad_info names no time tensor and
    keeps its count."""
    from dynamics_aware_diffusion_amd import _engine
    from dynamics_aware_diffusion_amd.utils.synth import unet_param_shapes
    lib = _engine.load_library()
    h = _model(lib)
    try:
        n, total = C.c_int32(), C.c_int64()
        assert lib.dad_train_time_grad_count(h, C.byref(n), C.byref(total)) == 0
        shapes = unet_param_shapes(6, 32, (1, 2, 4), 5, 32)
        keys, end = [], 0
        for i in range(n.value):
            key, off, numel = C.c_char_p(), C.c_int64(), C.c_int64()
            assert lib.dad_train_time_grad_info(h, i, C.byref(key), C.byref(off), C.byref(numel)) == 0
            k = key.value.decode()
            want = 1
            for d in shapes[k]:
                want *= d
            assert numel.value == want and off.value % 4 == 0 and off.value >= end, k
            end = off.value + numel.value
            keys.append(k)
        assert end <= total.value
        blocks = ["downs.0.0", "downs.0.1", "downs.1.0", "downs.1.1", "downs.2.0", "downs.2.1", "mid_block1", "mid_block2",
                  "ups.0.0", "ups.0.1", "ups.1.0", "ups.1.1"]
        assert keys == ["time_mlp.1.weight", "time_mlp.1.bias", "time_mlp.3.weight", "time_mlp.3.bias"] + \
            [f"{b}.time_mlp.1.{s}" for b in blocks for s in ("weight", "bias")]
        assert sorted(keys) == sorted(k for k in shapes if "time_mlp." in k)
        assert lib.dad_train_time_grad_info(h, n.value, None, None, None) == INVALID
        cn = C.c_int32()
        assert lib.dad_train_grad_count(h, C.byref(cn), None) == 0
        assert cn.value == len(shapes) - len(keys)
        for i in range(cn.value):
            key = C.c_char_p()
            assert lib.dad_train_grad_info(h, i, C.byref(key), None, None) == 0
            assert b"time_mlp." not in key.value
    finally:
        lib.dad_model_destroy(h)


def test_objective_workspace_extends_the_training_workspace():
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    h = _model(lib)
    try:
        for B in (1, 5, 9, 250, 256):
            sv, sc, osv, osc = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
            assert lib.dad_train_workspace_bytes(h, B, C.byref(sv), C.byref(sc)) == 0
            assert lib.dad_train_objective_workspace_bytes(h, B, C.byref(osv), C.byref(osc)) == 0
            # x_t and the output alone are 2 * B * H * td floats of `saved`; d out and the projections' gradient of `scratch`
            assert osv.value >= sv.value + 2 * B * 32 * 6 * 4 and osc.value >= sc.value + B * 32 * 6 * 4
            xt, out = C.c_size_t(), C.c_size_t()
            assert lib.dad_debug_objective_offsets(h, B, C.byref(xt), C.byref(out)) == 0
            assert sv.value <= xt.value < out.value < osv.value and xt.value % 16 == 0 and out.value % 16 == 0
        assert lib.dad_train_objective_workspace_bytes(h, 0, None, None) == INVALID
        assert lib.dad_train_objective_workspace_bytes(None, 4, None, None) == INVALID
    finally:
        lib.dad_model_destroy(h)


def test_argument_errors_are_invalid_with_a_message():
    """A null pointer, an unknown loss_type, training mode off, the split-f16 arithmetic: all DAD_E_INVALID, all
    before any device call (the models here are never finalized; the wrong-count refusal sits behind the state checks
    and is tested on a finalized model, tests/test_hip_objective.py)."""
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    one = (C.c_void_p * 1)(p)

    def fwd(h, loss_type=2, x0=p, t=p, noise=p, loss=p, saved=p):
        return lib.dad_train_objective_forward(h, x0, t, noise, None, loss_type, loss, 4, saved, 256, None)

    def bwd(h, loss_type=2, x0=p, d_loss=p, grads=one, n=1, tgrads=one, nt=1):
        return lib.dad_train_objective_backward(h, x0, p, None, loss_type, d_loss, grads, n, tgrads, nt, 4, p, 256, p, 256, None)

    h = _model(lib)
    try:
        assert fwd(None) == INVALID and b"null" in lib.dad_last_error()
        for kw in ({"x0": None}, {"t": None}, {"noise": None}, {"loss": None}, {"saved": None}):
            assert fwd(h, **kw) == INVALID and b"null pointer" in lib.dad_last_error(), kw
        for kw in ({"x0": None}, {"d_loss": None}, {"grads": None}, {"tgrads": None}):
            assert bwd(h, **kw) == INVALID and b"null pointer" in lib.dad_last_error(), kw
        for lt in (0, 3, -1):
            assert fwd(h, loss_type=lt) == INVALID and b"loss_type" in lib.dad_last_error()
            assert bwd(h, loss_type=lt) == INVALID and b"loss_type" in lib.dad_last_error()
        assert lib.dad_model_load_train_schedule(h, None, p, 20) == INVALID
        assert lib.dad_model_load_train_schedule(h, p, p, 19) == INVALID and b"19" in lib.dad_last_error()
        assert lib.dad_model_load_train_schedule(h, p, p, 20) == 0          # (host copy only: not finalized)
        # not finalized: a state error, not a crash
        assert fwd(h) == -2 and b"finalize" in lib.dad_last_error()
    finally:
        lib.dad_model_destroy(h)
    h = _model(lib, training=False)
    try:
        assert fwd(h) == INVALID and b"training mode is off" in lib.dad_last_error()
        assert bwd(h) == INVALID and b"training mode is off" in lib.dad_last_error()
        assert lib.dad_model_set_precision(h, 1) == 0
        assert lib.dad_model_set_training(h, 1) == INVALID               # (as before: no split-f16 training)
    finally:
        lib.dad_model_destroy(h)
    # split-f16 selected after training mode: the objective refuses it itself
    h = _model(lib)
    try:
        assert lib.dad_model_set_precision(h, 1) == 0
        assert fwd(h) == INVALID and b"split-f16" in lib.dad_last_error()
        assert bwd(h) == INVALID and b"split-f16" in lib.dad_last_error()
    finally:
        lib.dad_model_destroy(h)


def test_objective_plan_needs_training_and_a_batch():
    import pytest
    from dynamics_aware_diffusion_amd._engine import DadError, HipEngine
    eng = HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20)
    with pytest.raises(DadError, match="dad_model_set_training"):
        eng.objective_plan(4)
    eng = HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20, training=True)
    for bad in (0, -3):
        with pytest.raises(DadError):
            eng.objective_plan(bad)
    need = C.c_int32()
    assert eng.lib.dad_debug_objective_plan(None, 4, None, 0, C.byref(need)) == INVALID
    assert eng.lib.dad_debug_objective_plan(eng._h, 4, None, 5, C.byref(need)) == INVALID      # capacity without a buffer
    # a short buffer is filled as far as it goes and the full length is reported
    buf = (C.c_int32 * 8)()
    assert eng.lib.dad_debug_objective_plan(eng._h, 4, buf, 8, C.byref(need)) == 0
    assert need.value == 8 + 9 * 11 and buf[6] == 11 and buf[7] == 9


def test_objective_plan_of_one_hand_computed_case():
    """The tiny net (dim = time_dim = 32, channels 32 / 64 / 128: temb_width = 4 * 224 = 896) at batch 250, worked out
    from the kernel's own statement (32 x 32 output tiles, 32-wide K chunks): ceil(250 / 32) = 8 row tiles, 250 = 7 * 32
    + 26 as K.  d act = d rows . W: 8 x 1 output tiles, so min(256 / 8, 896 / 128) = 7 slices of 128 columns."""
    from dynamics_aware_diffusion_amd._engine import TIME_GEMM_MODES, HipEngine
    eng = HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20, training=True)
    p = eng.objective_plan(250)
    assert {k: v for k, v in p.items() if k != "launches"} == {
        "loss_blocks": 47, "kslices": 7, "kslice": 128, "temb_width": 896, "blocks": 12, "n": 250 * 32 * 6}
    want = [  # mode, M, N, K, grid, chunks, last_chunks, ktail, kslice
        ("FWD_H1", 250, 128, 32, (8, 4, 1), 1, 1, 0, 32),
        ("FWD_TEMB", 250, 32, 128, (8, 1, 1), 4, 4, 0, 128),
        ("FWD_ROWS", 250, 896, 32, (8, 28, 1), 1, 1, 0, 32),
        ("BWD_DWK", 896, 32, 250, (28, 1, 1), 8, 8, 26, 250),
        ("BWD_DACT", 250, 32, 896, (8, 1, 7), 4, 4, 0, 128),
        ("DTEMB", 250, 32, 7, (32, 1, 1), 0, 0, 0, 7),
        ("BWD_DW3", 32, 128, 250, (1, 4, 1), 8, 8, 26, 250),
        ("BWD_DH1", 250, 128, 32, (8, 4, 1), 1, 1, 0, 32),
        ("BWD_DW1", 128, 32, 250, (4, 1, 1), 8, 8, 26, 250),
    ]
    fields = ("mode", "M", "N", "K", "grid", "chunks", "last_chunks", "ktail", "kslice")
    assert len(p["launches"]) == 9 and len(TIME_GEMM_MODES) == 9
    for got, w in zip(p["launches"], want):
        assert got == dict(zip(fields, w)), (got, w)
    # the grids multiply out to the 32 x 32 tiles of every output (and the slab sum's 256 elements per block)
    blocks = sum(q["grid"][0] * q["grid"][1] * q["grid"][2] for q in p["launches"])
    assert blocks == 32 + 8 + 224 + 28 + 56 + 32 + 4 + 32 + 4
    # the loss's partial sums: one block per 1024 elements, at most 1024 of them
    assert eng.objective_plan(1)["loss_blocks"] == 1 and eng.objective_plan(1)["n"] == 192
    big = HipEngine(transition_dim=17, dim=32, channels=(32, 64), horizon=128, n_timesteps=20, training=True).objective_plan(512)
    assert big["n"] == 512 * 128 * 17 > 1 << 20 and big["loss_blocks"] == 1024


def test_engine_gradient_lists_are_disjoint():
    """What the Python binding passes as grad_tensors / time_grad_tensors: two lists without a common key (the
    wrong-count refusal needs a finalized model: tests/test_hip_objective.py)."""
    from dynamics_aware_diffusion_amd import _engine
    eng = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=20, training=True)
    conv, _ = eng.grad_layout()
    time, _ = eng.time_grad_layout()
    assert len(time) == 4 + 2 * 12 and len(conv) > 0
    assert not {k for k, _, _ in conv} & {k for k, _, _ in time}


def test_flag_defaults_to_off():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    diff = GaussianDiffusion(TemporalUnet(6, dim=32, dim_mults=(1, 2)), 32, 4, 2, n_timesteps=20)
    assert diff.fused_objective is False


def test_objective_layout_under_address_and_ub_sanitizers(tmp_path):
    """tests/sanitize/objective_check.cpp: regions disjoint, 16-byte aligned, inside the reported sizes, the K slices
    of the time chain's backward cover temb_width once — compiled host-only with -fsanitize=address,undefined."""
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "objective_check"
    src = os.path.join(ROOT, "tests", "sanitize", "objective_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "objective host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
