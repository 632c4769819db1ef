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
               "dad_debug_objective_offsets")


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
