"""CPU tests (`-m "not gpu"`) of horizons above 128 positions: the library accepts nets whose layers are longer than
any whole-sample tile (windowed tiles + the GroupNorm pass, csrc/conv_gemm.hpp WIN / csrc/conv_gn_pass.hpp), keeps
the refusals it had, and the windowed launches satisfy the kernels' invariants (tests/sanitize/long_horizon_check.cpp
under the address / UB sanitizers)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(td, dim, mults, horizon, ks=5, channels=None):
    from dynamics_aware_diffusion_amd import _engine
    cfg = _engine.DadCfg()
    cfg.transition_dim, cfg.dim, cfg.time_dim, cfg.n_levels = td, dim, dim, len(mults)
    for i, ch in enumerate(channels or [dim * k for k in mults]):
        cfg.channels[i] = ch
    cfg.kernel_size, cfg.horizon, cfg.n_timesteps = ks, horizon, 20
    cfg.predict_epsilon = cfg.clip_denoised = 1
    return cfg


# (id, transition_dim, dim, mults, padded horizon, kernel_size, real horizon or None, padded level widths or None)
LONG_NETS = [
    ("H256_dim32_148", 6, 32, (1, 4, 8), 256, 5, None, None),
    ("H512_dim32_148", 6, 32, (1, 4, 8), 512, 5, None, None),
    ("H256_dim64_124", 6, 64, (1, 2, 4), 256, 5, None, None),
    ("H256_dim128_1248", 6, 128, (1, 2, 4, 8), 256, 5, None, None),
    ("H200_pointmaze", 6, 128, (1, 2, 4), 256, 5, 200, None),
    ("H384_dim32_148", 6, 32, (1, 4, 8), 512, 5, 384, None),
    ("H256_k3", 6, 32, (1, 2, 4), 256, 3, None, None),
    ("H512_k7", 5, 32, (1, 2, 4), 512, 7, None, None),
    ("H256_dim96_padded", 6, 128, (1, 2, 4), 256, 5, None, (96, 192, 384)),
]


@pytest.mark.parametrize("net", LONG_NETS, ids=lambda n: n[0])
def test_long_horizon_nets_are_accepted(net):
    """Every layer of these nets is 256 or 512 positions long somewhere: before windowed tiles the library refused
    them at dad_model_create ("no tile configuration for downs.0.0.blocks.0.block.0 ... L=256")."""
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    _, td, dim, mults, H, ks, hreal, real = net
    h = C.c_void_p()
    rc = lib.dad_model_create(C.byref(_cfg(td, dim, mults, H, ks)), C.byref(h))
    assert rc == 0, lib.dad_last_error()
    try:
        if hreal is not None:
            assert lib.dad_model_set_horizon(h, hreal) == 0, lib.dad_last_error()
        if real is not None:
            arr = (C.c_int32 * len(real))(*real)
            assert lib.dad_model_set_group_channels(h, arr, len(real)) == 0, lib.dad_last_error()
        for B in (1, 32, 256):
            n = C.c_size_t()
            assert lib.dad_workspace_bytes(h, B, C.byref(n)) == 0 and n.value > 0
        # batch 1 runs the batch kernels: the small-batch plan keeps refusing horizons above 128
        launches, wide = C.c_int32(), C.c_int32()
        assert lib.dad_debug_small_batch_plan(h, 1, C.byref(launches), C.byref(wide)) == 0
        assert launches.value == 0
        # split-f16 sampling is accepted (the windowed layers run fp32); training stays refused in f16x3 as before
        # and is accepted in fp32 (windowed data- and weight-gradient kernels)
        assert lib.dad_model_set_precision(h, 1) == 0
        assert lib.dad_model_set_training(h, 1) == -1
        assert b"fp32" in lib.dad_last_error()
        assert lib.dad_model_set_precision(h, 0) == 0
        assert lib.dad_model_set_training(h, 1) == 0, lib.dad_last_error()
        for B in (1, 3, 64):
            saved, scratch = C.c_size_t(), C.c_size_t()
            assert lib.dad_train_workspace_bytes(h, B, C.byref(saved), C.byref(scratch)) == 0
            assert saved.value > 0 and scratch.value > 0
    finally:
        lib.dad_model_destroy(h)


def test_existing_refusals_stay():
    """Windowed tiles widen nothing else: H = 12 on four levels, GroupNorm(8, 44), kernel sizes 4 / 9 / 1 and the
    2048-channel groups at a windowed length stay refused."""
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    h = C.c_void_p()
    assert lib.dad_model_create(C.byref(_cfg(6, 32, (1, 2, 2, 4), 12)), C.byref(h)) == -1
    assert lib.dad_model_create(C.byref(_cfg(6, 32, (1, 2, 4), 256, channels=(32, 44, 128))), C.byref(h)) == -1
    for ks in (4, 9, 1):
        assert lib.dad_model_create(C.byref(_cfg(6, 32, (1, 2, 4), 256, ks=ks)), C.byref(h)) == -1
    assert lib.dad_model_create(C.byref(_cfg(6, 2048, (1, 2), 256)), C.byref(h)) == -1
    assert b"no tile configuration" in lib.dad_last_error()


def test_python_engine_pads_long_horizons():
    """The Python mirror pads 200 / 384 up to 256 / 512 and keeps the trajectory at its real length."""
    from dynamics_aware_diffusion_amd import _engine
    for H, want in ((200, 256), (384, 512), (256, 256), (500, 512)):
        eng = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=H, n_timesteps=10)
        assert eng.padded_horizon == want and eng.horizon == H and eng.rows_padded == (H != want)


def test_windowed_launch_invariants_under_address_and_ub_sanitizers(tmp_path):
    """tests/sanitize/long_horizon_check.cpp: window coverage, halos inside the sample, X stage / LDS sizing, split-K
    tickets and slabs against the workspace for every batch the planner admits — compiled host-only with
    -fsanitize=address,undefined."""
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "long_horizon_check"
    src = os.path.join(ROOT, "tests", "sanitize", "long_horizon_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "long horizon host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
