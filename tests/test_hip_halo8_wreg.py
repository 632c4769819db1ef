"""The register-weight form of the halo-skipping kernel (csrc/conv_halo8.hpp, conv_halo8w_f32): the
same products in the same order as conv_halo8_f32 with the weights read global -> register -> MFMA, so every output is
BIT-EQUAL between the two forms.  The option "halo8_wreg" picks the form: 1 every launch, 0 none, -1 the default.

Net and batches are tests/test_hip_halo8_paths.py's first case — d64 (1, 2) H16 at batch 889, the first batch whose plan
holds all four instantiations ("halo8", tile, ride) at once: 889 = 111 tiles of eight samples and one sample more (the
last tile has nvalid = 1); 896 fills the last tile.

Host (no device): the plan names the form of every launch (forward_plan: ``wreg``), all four keys in both forms; the
program tests/sanitize/halo8w_check.cpp under the address / UB sanitizers: the kernel's address arithmetic repeated.
GPU: unet_forward (shared timestep), unet_forward_rows (per-row timesteps) and a 2-step sample_loop, option on against off.
"""
import functools
import os
import subprocess
import shutil

import pytest
import torch

from tests import fullchip_census as census
from tests.test_hip_parity import dev  # noqa: F401  (fixture)
from tests.util import as_torch  # noqa: F401

TD, DIM, MULTS, H, T = 6, 64, (1, 2), 16, 20
FORMS = {("halo8", tile, ride) for tile in (0, 1) for ride in (0, 1)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wreg(eng, value):
    """The option, through the library directly (an engine without a device has no current device to synchronise)."""
    from dynamics_aware_diffusion_amd._engine import _check
    _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, b"halo8_wreg", int(value)))


def _forms(eng, B, mode):
    """{key: {wreg of its launches}} over the halo8 launches of the plan the engine reports."""
    out = {}
    for q in eng.forward_plan(B, mode)["launches"]:
        if q["key"][0] == "halo8":
            out.setdefault(q["key"], set()).add(q["wreg"])
    return out


# ------------------------------------------------------------------------------------------------ host
def test_plan_names_the_form_of_every_launch():
    eng = census.host_engine(TD, DIM, MULTS, H, 5, "fp32")
    census.set_all(eng, {})
    for B in (889, 896):
        for mode in (0, 1):
            default = _forms(eng, B, mode)
            assert set(default) == FORMS, (B, mode, sorted(default))
            assert all(len(v) == 1 for v in default.values()), "one default per (tile, ride)"
            try:
                _wreg(eng, 1)
                assert _forms(eng, B, mode) == {k: {True} for k in FORMS}
                _wreg(eng, 0)
                assert _forms(eng, B, mode) == {k: {False} for k in FORMS}
                # the report of conv_halo8_f32's operands is the same for both forms
                off = eng.halo8_plan(B, mode)
                _wreg(eng, 1)
                assert eng.halo8_plan(B, mode) == off and off
            finally:
                _wreg(eng, -1)
            assert _forms(eng, B, mode) == default
    # below the full-chip rule nothing takes either form
    assert not _forms(eng, 64, 1)


def test_address_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "halo8w_check"
    src = os.path.join(ROOT, "tests", "sanitize", "halo8w_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "halo8w_check: ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _inputs():
    """Weights, inputs, timesteps and noise; nobody writes into them."""
    from dynamics_aware_diffusion_amd.utils import synth
    from tests.test_hip_halo8_paths import _timesteps
    state = synth.synth_unet_state(TD, DIM, MULTS, seed=61, affine_jitter=0.3)
    x = torch.from_numpy(synth.normal_like(37, "halo8w.x", (896, H, TD)))
    t = torch.from_numpy(_timesteps("halo8w", 896))
    noise = torch.from_numpy(synth.normal_like(37, "halo8w.noise", (3, 889, H, TD)))
    cond = torch.zeros(1, TD)
    cond[0, :TD - 1] = torch.from_numpy(synth.uniform(37, "halo8w.cond", (TD - 1,), 0.9))
    return {"state": state, "x": x, "t": t, "noise": noise, "cond": cond}


@functools.lru_cache(maxsize=None)
def _engine(dev):
    from tests.test_hip_long_horizon import _diffusion
    diff = _diffusion(TD, TD - 1, 1, DIM, MULTS, H, T, _inputs()["state"], dev)
    return diff, diff._engine(dev)


def _both(eng, B, mode, run):
    """run() under halo8_wreg = 1 and 0, each on the plan that says so for all four forms."""
    got = {}
    try:
        for on in (1, 0):
            _wreg(eng, on)
            assert _forms(eng, B, mode) == {k: {bool(on)} for k in FORMS}, (B, mode, on)
            got[on] = run()
    finally:
        _wreg(eng, -1)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("B,mode", [(889, 0), (896, 0), (889, 1), (896, 1)],
                         ids=["part_tile", "full_tile", "part_tile_per_row", "full_tile_per_row"])
def test_forward_bit_equal_between_the_forms(B, mode, dev):
    inp = _inputs()
    _, eng = _engine(dev)
    x, t = inp["x"][:B].to(dev).contiguous(), inp["t"][:B].to(dev).contiguous()
    got = _both(eng, B, mode, lambda: (eng.unet_forward_rows(x, t) if mode == 1 else eng.unet_forward(x, 7)).cpu())
    assert torch.isfinite(got[1]).all() and float(got[1].abs().max()) > 0
    differ = int((got[1] != got[0]).sum())
    print(f"\nB={B} mode={mode}: {differ} of {got[1].numel()} outputs differ, max |d| = {float((got[1] - got[0]).abs().max()):.2e}")
    assert torch.equal(got[1], got[0])


@pytest.mark.gpu
def test_sample_loop_bit_equal_between_the_forms(dev):
    inp = _inputs()
    _, eng = _engine(dev)
    B, steps = 889, 2
    noise, cond = inp["noise"].to(dev), inp["cond"].to(dev)

    def run():
        x = noise[0].clone()
        x[:, 0] = cond
        eng.sample_loop(x, steps, noise_stack=noise[1:].contiguous(), cond0=cond)
        torch.cuda.synchronize()
        return x.cpu()

    got = _both(eng, B, 0, run)
    assert torch.isfinite(got[1]).all()
    assert torch.equal(got[1], got[0])
