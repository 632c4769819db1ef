"""The seam between two denoise steps of dad_sample_loop as one launch (csrc/conv_seam.hpp): the posterior
update of step t and the first conv of the evaluation at t - 1.

Host (no device): tests/sanitize/seam_check.cpp under the address / UB sanitizers -- the rule over a sweep, the kernel's
LDS arithmetic, a simulated X stage against the conv, the unit left out, the epilogue ownership --; the report
(HipEngine.seam_plan) says "taken" under the rule's conditions and names the first condition that fails otherwise; the
records of plan_forward do not depend on the option.

GPU, option "cc" off so that small batches take the batch kernels, transition_dim 6 (one 8-channel unit) and 16 (two):
  d32_m1_H8_B5     four samples per 32-row tile, the last tile holds one; tile 0
  d64_m12_H16_B3   two samples per tile, the second tile half filled; tile 0
  d128_m1_H32_B3   the headline's first-layer shape, one sample per tile; tile 0, a (sample, group) pair spans a wave
  d64_m1_H16_B893  the smallest batch that puts the 64-channel first conv on tile 1 (224 blocks)
  d128_m1_H32_B223 the same for 128 channels: the headline's first-layer shape on the headline's tile, a full-chip grid
x after sample_loop with the seam on is BIT-EQUAL to x
with it off for n_steps 1, 2 and 5 x (injected noise, Philox at row_offset 2^27 + 3) x (no condition, shared, per row) x
predict_epsilon 0 / 1 x clip_denoised 0 / 1; a second call gives the same bits; graph replay equals eager; one case
against oracle.sample_loop at TOL_LOOP.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import forward_census as census
from tests.test_hip_parity import TOL_LOOP, dev  # noqa: F401  (dev: fixture)
from tests.util import as_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 20
# (id, dim, mults, horizon, batch, tile of the first conv)
NETS = [
    ("d32_m1_H8_B5", 32, (1,), 8, 5, 0),
    ("d64_m12_H16_B3", 64, (1, 2), 16, 3, 0),
    ("d128_m1_H32_B3", 128, (1,), 32, 3, 0),
    ("d64_m1_H16_B893", 64, (1,), 16, 893, 1),
    ("d128_m1_H32_B223", 128, (1,), 32, 223, 1),
]
TDS = (6, 16)
ROW_OFFSET = 2 ** 27 + 3


# ------------------------------------------------------------------------------------------------ host
def test_seam_host_logic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "seam_check"
    src = os.path.join(ROOT, "tests", "sanitize", "seam_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "seam host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def _host(td=6, dim=128, mults=(1, 2, 4), H=32, ks=5, precision="fp32", **options):
    eng = census.host_engine(td, dim, mults, H, ks, precision)
    census.set_options(eng, options.pop("tile", -1), dict({"cc": 0}, **options))
    return eng


def test_report_says_taken_under_the_rule_and_names_every_refusal():
    from dynamics_aware_diffusion_amd._engine import _check
    head = _host().seam_plan(256)
    assert head == {"taken": True, "reason": "taken", "grid": 256, "threads": 512, "tile": 1, "units": 1,
                    "lds_bytes": 4 * (2 * 32 * 132 + 6 * 128 + 8 + 36 * 20 + 64)}, head
    assert _host().seam_plan(256, detail=True) == dict(head, spt=1, last=1, buffers="dst", dim=128, tile0=0)
    for name, dim, mults, H, B, tile in NETS:
        for td in TDS:
            q = _host(td, dim, mults, H).seam_plan(B)
            assert q["taken"] and q["tile"] == tile and q["units"] == (1 if td <= 8 else 2), (name, td, q)
            assert q["grid"] == (B * H + 31) // 32 and q["threads"] == 4 * dim and q["lds_bytes"] <= 160 * 1024
            q = _host(td, dim, mults, H).seam_plan(B, detail=True)
            assert q["spt"] == 32 // H and (q["grid"] - 1) * q["spt"] + q["last"] == B and 1 <= q["last"] <= q["spt"]
            assert q["dim"] == dim and q["tile0"] == (tile == 0) and q["buffers"] in ("dst", "rdst", "apart")
    # the first tile-1 batches are what NETS says
    assert _host(6, 64, (1,), 16).seam_plan(892)["tile"] == 0 and _host(6, 128, (1,), 32).seam_plan(222)["tile"] == 0
    refusals = [
        ("option off", _host(), 256, False, "step_seam"),
        ("small-batch kernels", _host(cc=1), 3, False, None),
        ("split-f16 arithmetic", _host(precision="f16x3"), 256, False, None),
        ("forced tile", _host(tile=0), 256, False, None),
        ("forced tile", _host(tile=99), 256, False, None),
        ("projection", _host(), 256, True, None),
        ("zero-padded net", _host(H=24), 256, False, None),
        ("horizon", _host(H=64), 256, False, None),
        ("transition_dim", _host(td=17), 256, False, None),
        ("dim", _host(dim=256, mults=(1, 2)), 256, False, None),
        ("first conv", _host(ks=3), 256, False, None),
        ("no riding residual conv", _host(fuse_residual=0), 256, False, None),
        ("tile", _host(), 1024, False, None),      # 512 N tiles: the 128-channel tile, eight float4 per thread
    ]
    for reason, eng, B, proj, off in refusals:
        if off:
            _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, off.encode(), 0))
        q = eng.seam_plan(B, projection=proj)
        assert q == {"taken": False, "reason": reason, "grid": 0, "threads": 0, "lds_bytes": 0, "tile": -1, "units": 0}, (reason, q)
        assert eng.seam_plan(B, projection=proj, detail=True) == dict(q, spt=0, last=0, buffers=None, dim=0, tile0=-1), reason
    # each of them alone decides: the same engines are taken once the condition is lifted
    assert _host(td=16).seam_plan(256)["taken"] and _host(H=16).seam_plan(256)["taken"] and _host(dim=64).seam_plan(256)["taken"]
    assert _host(cc=1).seam_plan(256)["taken"], "batch 256 takes the batch kernels whatever the option"


def test_forward_plan_records_do_not_depend_on_the_option():
    from dynamics_aware_diffusion_amd._engine import _check
    for name, dim, mults, H, B, _ in NETS:
        eng = _host(6, dim, mults, H)
        plans = {}
        for on in (1, 0):
            _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, b"step_seam", on))
            assert eng.seam_plan(B)["taken"] == bool(on)
            plans[on] = [eng.forward_plan(b, mode) for b in (B, 256) for mode in (0, 1)]
        assert plans[0] == plans[1], name


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _inputs(name, td):
    """Weights, start, injected noise and conditions of a net; nobody writes into them."""
    from dynamics_aware_diffusion_amd.utils import synth
    _, dim, mults, H, B, _ = next(n for n in NETS if n[0] == name)
    state = synth.synth_unet_state(td, dim, mults, seed=53, affine_jitter=0.3)
    noise = torch.from_numpy(synth.normal_like(37, f"seam.noise.{name}.{td}", (6, B, H, td)))
    cond = torch.from_numpy(synth.uniform(37, f"seam.cond.{name}.{td}", (B, td), 0.9))
    return {"state": state, "noise": noise, "cond": cond}


def _engine(net, td, dev, **kw):
    from tests.test_hip_long_horizon import _diffusion
    name, dim, mults, H, B, tile = net
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, _inputs(name, td)["state"], dev, **kw)
    eng = diff._engine(dev)
    eng.debug_set_option("cc", 0)
    q = eng.seam_plan(B)
    assert q["taken"] and q["tile"] == tile, (name, td, q)
    return diff, eng


def _loop(eng, inp, dev, n_steps, noise_mode, cond_mode, **kw):
    x = inp["noise"][0].to(dev).clone()
    cond = {"none": None, "shared": inp["cond"][:1], "rows": inp["cond"]}[cond_mode]
    if cond is not None:
        cond = cond.to(dev).contiguous()
        x[:, 0] = cond
    if noise_mode == "injected":
        eng.sample_loop(x, n_steps, noise_stack=inp["noise"][1:1 + n_steps].to(dev).contiguous(), cond0=cond, **kw)
    else:
        eng.sample_loop(x, n_steps, seed=0x123456789ABCDEF, row_offset=ROW_OFFSET, cond0=cond, **kw)
    torch.cuda.synchronize()
    return x.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("td", TDS)
@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_seam_on_is_bit_equal_to_seam_off(net, td, dev):
    inp = _inputs(net[0], td)
    worst = 0.0
    for pe in (1, 0):
        for clip in (1, 0):
            diff, eng = _engine(net, td, dev, predict_epsilon=bool(pe), clip_denoised=bool(clip))
            try:
                for n_steps in (1, 2, 5):
                    for noise_mode in ("injected", "philox"):
                        for cond_mode in ("none", "shared", "rows"):
                            got = {}
                            for on in (1, 0):
                                eng.debug_set_option("step_seam", on)
                                got[on] = _loop(eng, inp, dev, n_steps, noise_mode, cond_mode)
                            assert torch.isfinite(got[1]).all()
                            d = float((got[1] - got[0]).abs().max())
                            worst = max(worst, d)
                            assert torch.equal(got[1], got[0]), (net[0], td, pe, clip, n_steps, noise_mode, cond_mode, d)
            finally:
                eng.debug_set_option("step_seam", 1)
            assert diff.model._engine is eng
    print(f"\n{net[0]} td={td}: max |seam on - seam off| = {worst:.1e}")


@pytest.mark.gpu
@pytest.mark.parametrize("net", NETS, ids=lambda n: n[0])
def test_seam_second_call_and_graph_replay_give_the_same_bits(net, dev):
    td = 6
    inp = _inputs(net[0], td)
    _, eng = _engine(net, td, dev)
    for noise_mode in ("injected", "philox"):
        first = _loop(eng, inp, dev, 5, noise_mode, "shared")
        assert torch.equal(first, _loop(eng, inp, dev, 5, noise_mode, "shared")), "a second call gives other bits"
        graph = _loop(eng, inp, dev, 5, noise_mode, "shared", use_graph=True)
        assert torch.equal(first, graph), "graph replay differs from eager"
        assert torch.equal(graph, _loop(eng, inp, dev, 5, noise_mode, "shared", use_graph=True)), "a second replay gives other bits"


@pytest.mark.gpu
def test_seam_loop_vs_oracle(dev):
    """The last 5 reverse steps of the T = 20 schedule (a truncated loop, as the loop cases of tests/test_hip_parity.py)
    with injected noise and an inpainted first row, on the headline's first-layer shape."""
    from oracle import denoiser as orc
    net, td, steps = NETS[2], 6, 5
    inp = _inputs(net[0], td)
    cond = inp["cond"][:1]
    want = orc.sample_loop(as_torch(inp["state"]), orc.schedule_buffers("cosine", T), inp["noise"], steps, {0: cond})
    _, eng = _engine(net, td, dev)
    got = _loop(eng, inp, dev, steps, "injected", "shared")
    err = float((got - want).abs().max())
    print(f"\nseam loop {net[0]} T={steps}: |hip - oracle| = {err:.2e}")
    assert np.isfinite(err) and err <= TOL_LOOP
