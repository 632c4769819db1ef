"""The halo-skipping kernel of 8-position 5-tap convs (csrc/conv_halo8.hpp).

Host (no device): tests/sanitize/halo8_check.cpp under the address / UB sanitizers — slot shifts, bank conflicts of every
fragment read, a simulated stage against the conv, the products left out, the planner's rule — and the plan of a
forced-tile engine, which holds no key of the family.

GPU: the kernel with the "halo8" option on, and the conv-GEMM kernels with it off, against the float64 oracle at the
forward tests' gate (tests/test_hip_long_horizon.py: <= TOL_STEP from the fp32 oracle and no farther from float64 than
twice the fp32 oracle, + 5e-7), at the smallest batches the planner takes the kernel at:
  d32_m124_H32        the first batch whose plan holds the family (313: 40 N tiles x 4 M tiles of tile 0 = 160 tiles, no
                      grid split-K), 128 channels at 8 positions; 64 -> 128 carries the riding 1x1 conv; the last N tile
                      holds one sample of eight
  d32_m124_H32_part   the same + 3: four samples in the last N tile (both are partly empty: neither 313 nor 316 is a
                      multiple of 8; a full last tile runs in tests/test_hip_halo8_paths.py)
  d32_m14_H16_tile1   the first batch that takes it on tile 1 (889: 112 N tiles x 2 M tiles = 224 blocks), 32 -> 128 with
                      the ride in one K chunk, 128 -> 128 in four
  d32_m1_H8           horizon 8, one level: the first level is the 8-position one (32 -> 32, one K chunk, GroupNorm with
                      time embedding and residual, the final Conv1dBlock); 1273 = 160 N tiles of tile 0
plus a sampling loop of 4 steps at TOL_LOOP and a repeat that gives the same bits.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests.test_hip_parity import TOL_LOOP, TOL_STEP, dev  # noqa: F401  (dev: fixture)
from tests.util import as_torch, max_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 20
TD = 6
# (id, dim, mults, horizon, tile the family must be taken on, batch beyond the first that does)
NETS = [
    ("d32_m124_H32", 32, (1, 2, 4), 32, 0, 0),
    ("d32_m124_H32_part", 32, (1, 2, 4), 32, 0, 3),
    ("d32_m14_H16_tile1", 32, (1, 4), 16, 1, 0),
    ("d32_m1_H8", 32, (1,), 8, 0, 0),
]


def _halo8_keys(plan):
    return sorted({q["key"] for q in plan["launches"] if q["key"][0] == "halo8"})


@functools.lru_cache(maxsize=None)
def _first_batch(dim, mults, H, tile):
    """The smallest batch whose shared-timestep plan takes the family on `tile` (host logic only)."""
    from dynamics_aware_diffusion_amd._engine import HipEngine
    eng = HipEngine(transition_dim=TD, dim=dim, channels=[dim * k for k in mults], horizon=H, n_timesteps=T)
    for B in range(1, 4097):
        if any(k[1] == tile for k in _halo8_keys(eng.forward_plan(B, 0))):
            return B
    raise AssertionError(f"no batch up to 4096 takes conv_halo8_f32 on tile {tile}")


def test_halo8_host_logic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "halo8_check"
    src = os.path.join(ROOT, "tests", "sanitize", "halo8_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "halo8 host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_forced_tile_plans_hold_no_halo8_kernel():
    """A forced tile (split-K switched off included) pins the conv-GEMM kernels and their summation order; so does the
    option.  The first batches are what the module docstring says."""
    from dynamics_aware_diffusion_amd._engine import HipEngine
    assert [_first_batch(d, m, H, tile) for _, d, m, H, tile, _ in NETS] == [313, 313, 889, 1273]
    eng = HipEngine(transition_dim=TD, dim=32, channels=[32, 64, 128], horizon=32, n_timesteps=T)
    for B in (313, 889, 2048):
        for mode in (0, 1):
            keys = _halo8_keys(eng.forward_plan(B, mode))
            # (from 889 on the 128-channel launches run on tile 1; the decoder's 64-channel ones follow later)
            assert {k[1] for k in keys} in (({0},) if B < 889 else ({0, 1}, {1})), (B, mode, keys)
            assert ("halo8", 0 if B < 889 else 1, 1) in keys, "64 -> 128 carries the riding 1x1 conv"
        for tile in (0, 1, 2, 4, 99, 100, 101):
            eng.lib.dad_debug_set_tile(eng._h, tile)
            assert not _halo8_keys(eng.forward_plan(B, 1)), (B, tile)
        eng.lib.dad_debug_set_tile(eng._h, -1)
        eng.lib.dad_debug_set_option(eng._h, b"halo8", 0)
        assert not _halo8_keys(eng.forward_plan(B, 1))
        eng.lib.dad_debug_set_option(eng._h, b"halo8", 1)
        assert _halo8_keys(eng.forward_plan(B, 1))
    assert not _halo8_keys(eng.forward_plan(312, 0)) and not _halo8_keys(eng.forward_plan(4, 1))
    train = HipEngine(transition_dim=TD, dim=32, channels=[32, 64, 128], horizon=32, n_timesteps=T, training=True)
    assert not _halo8_keys(train.forward_plan(889, 2)) and not _halo8_keys(train.forward_plan(889, 3))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Weights, input and the oracle's fp32 / float64 forward of a net; nobody writes into it."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    _, dim, mults, H, tile, extra = next(n for n in NETS if n[0] == name)
    B = _first_batch(dim, mults, H, tile) + extra
    state = synth.synth_unet_state(TD, dim, mults, seed=47, affine_jitter=0.3)
    w = as_torch(state)
    x = torch.from_numpy(synth.normal_like(29, "halo8.x." + name, (B, H, TD)))
    tt = torch.full((B,), 7, dtype=torch.long)
    with torch.no_grad():
        out32 = orc.unet_forward(w, x, tt).numpy()
        out64 = orc.unet_forward(orc.cast_weights(w, torch.float64), x.double(), tt).numpy()
    return {"state": state, "B": B, "x": x, "out32": out32, "out64": out64, "o64": max_abs(out32, out64)}


@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_halo8_forward_vs_float64(net, dev):
    from tests.test_hip_long_horizon import _diffusion
    name, dim, mults, H, tile, _ = net
    ref = _oracle(name)
    B = ref["B"]
    diff = _diffusion(TD, TD - 1, 1, dim, mults, H, T, ref["state"], dev)
    eng = diff.model.engine(H, dev)
    x = ref["x"].to(dev)
    got = {}
    try:
        for on in (1, 0):
            eng.debug_set_option("halo8", on)
            keys = _halo8_keys(eng.forward_plan(B, 0))
            assert (any(k[1] == tile for k in keys) if on else not keys), (name, B, on, keys)
            got[on] = eng.unet_forward(x, 7).cpu().numpy()
            if on:
                assert np.array_equal(got[on], eng.unet_forward(x, 7).cpu().numpy()), "a second call gives other bits"
            assert diff.model._engine is eng
    finally:
        eng.debug_set_option("halo8", 1)
    for on in (1, 0):
        e32, e64 = max_abs(got[on], ref["out32"]), max_abs(got[on], ref["out64"])
        print(f"\n{name} B={B} halo8={on}: |hip-orc32|={e32:.2e} |hip-fp64|={e64:.2e} |orc32-fp64|={ref['o64']:.2e}")
        assert np.isfinite(got[on]).all()
        assert e32 <= TOL_STEP, (name, on)
        assert e64 <= 2 * ref["o64"] + 5e-7, (name, on)
    print(f"{name}: |halo8 - conv-GEMM| = {max_abs(got[1], got[0]):.2e}")


@pytest.mark.gpu
def test_halo8_result_does_not_depend_on_the_column_of_a_sample(dev):
    """A sample gives the same bits in whichever column of whichever tile it sits (rolled batch), and in a partly empty
    tile."""
    from tests.test_hip_long_horizon import _diffusion
    ref = _oracle("d32_m124_H32_part")
    B = ref["B"]
    diff = _diffusion(TD, TD - 1, 1, 32, (1, 2, 4), 32, T, ref["state"], dev)
    eng = diff.model.engine(32, dev)
    assert _halo8_keys(eng.forward_plan(B, 0))
    x = ref["x"].to(dev)
    a = eng.unet_forward(x, 7)
    b = eng.unet_forward(torch.roll(x, 5, 0).contiguous(), 7)
    assert torch.equal(torch.roll(a, 5, 0), b)


@pytest.mark.gpu
def test_halo8_sampling_loop_vs_oracle(dev):
    """The last 4 reverse steps of the T = 20 schedule (a truncated loop, as the loop cases of tests/test_hip_parity.py:
    a schedule of four steps in all has an eps gain of its own, which TOL_LOOP was not set for), with injected noise
    and an inpainted first row, at the first batch that takes the kernel."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    from tests.test_hip_long_horizon import _diffusion
    steps, dim, mults, H = 4, 32, (1, 2, 4), 32
    ref = _oracle("d32_m124_H32")
    B = ref["B"]
    w = as_torch(ref["state"])
    noise = torch.from_numpy(synth.normal_like(31, "halo8.loop", (steps + 1, B, H, TD)))
    cond = torch.zeros(1, TD)
    cond[0, :TD - 1] = torch.from_numpy(synth.uniform(31, "halo8.cond", (TD - 1,), 0.9))
    want = orc.sample_loop(w, orc.schedule_buffers("cosine", T), noise, steps, {0: cond})
    diff = _diffusion(TD, TD - 1, 1, dim, mults, H, T, ref["state"], dev)
    eng = diff._engine(dev)
    assert _halo8_keys(eng.forward_plan(B, 0))
    runs = []
    for _ in range(2):
        x = noise[0].to(dev).clone()
        x[:, 0] = cond.to(dev)
        eng.sample_loop(x, steps, noise_stack=noise[1:].to(dev).contiguous(), cond0=cond.to(dev))
        torch.cuda.synchronize()
        runs.append(x.cpu())
    err = float((runs[0] - want).abs().max())
    print(f"\nhalo8 loop B={B} T={steps}: |hip - oracle| = {err:.2e}")
    assert np.isfinite(err) and err <= TOL_LOOP
    assert torch.equal(runs[0], runs[1])
