"""The strided (DDIM) sampler's host side: no device.

* ``ddim_table`` against the float64 DDPM posterior of the same ``abar`` (eta = 1, every timestep), its timesteps, its
  first step, every refusal of ``ddim_table`` / ``set_sampler``;
* the sampler is plain data on ``GaussianDiffusion`` (deepcopy, pickle, ``state_dict``);
* ``dad_sampler_step`` / ``dad_sampler_loop`` refuse bad steps on a created, unfinalised model, before anything else;
* tests/sanitize/sampler_check.cpp (ancestral builder, validation, graph-key hash) under ASan + UBSan.
"""
import copy
import ctypes as C
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
from dynamics_aware_diffusion_amd import _engine
from dynamics_aware_diffusion_amd.models.diffusion import ddim_table, make_schedule, sampler_timesteps
from tests import forward_census as census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAD_E_INVALID, DAD_E_STATE, DAD_E_RANGE = -1, -2, -5


def _abar64(kind, T):
    return make_schedule(kind, T)["alphas_cumprod"].to(torch.float64).numpy()


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("kind,T", [("cosine", 20), ("cosine", 100), ("cosine", 1000), ("linear", 100)])
def test_eta_one_over_every_timestep_is_the_ddpm_posterior(kind, T):
    """1e-11: a hundred times the 1.3e-13 the two float64 forms differ by with glibc's libm."""
    abar = _abar64(kind, T)
    tab = ddim_table(make_schedule(kind, T)["alphas_cumprod"], T, 1.0)
    ap = np.concatenate([np.ones(1), abar[:-1]])
    alpha = abar / ap
    beta = 1.0 - alpha
    coef1 = beta * np.sqrt(ap) / (1.0 - abar)
    coef2 = (1.0 - ap) * np.sqrt(alpha) / (1.0 - abar)
    var = beta * (1.0 - ap) / (1.0 - abar)
    worst = max(np.abs(tab["coef_x0"] - coef1).max(), np.abs(tab["coef_xt"] - coef2).max(),
                np.abs(tab["sigma"] ** 2 - var).max(), np.abs(tab["sigma"] - np.sqrt(var)).max())
    print(f"{kind} T={T}: worst |ddim(eta=1) - ddpm| = {worst:.3e}")
    assert worst <= 1e-11
    assert np.array_equal(tab["tau"], np.arange(T))
    assert np.array_equal(tab["c_recip"], np.sqrt(1.0 / abar)) and np.array_equal(tab["c_recipm1"], np.sqrt(1.0 / abar - 1.0))
    assert np.array_equal(tab["guide_x0"], (1.0 - abar) / np.sqrt(abar)) and not tab["guide_mean"].any()
    assert all(tab[k].dtype == np.float64 and tab[k].shape == (T,) for k in _engine.SAMPLER_COEF_FIELDS)


def test_timesteps_of_K():
    T = 20
    assert sampler_timesteps(T, 1).tolist() == [0]
    assert sampler_timesteps(T, 5).tolist() == [0, 4, 8, 12, 16]
    assert sampler_timesteps(T, 7).tolist() == [0, 2, 5, 8, 11, 14, 17]
    assert sampler_timesteps(T, T).tolist() == list(range(T))
    assert sampler_timesteps(T, [0, 1, 3, 7, 19]).tolist() == [0, 1, 3, 7, 19]
    assert sampler_timesteps(1000, 7).tolist() == [i * 1000 // 7 for i in range(7)]
    assert ddim_table(_abar64("cosine", T), 7)["tau"].tolist() == [0, 2, 5, 8, 11, 14, 17]


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("steps", [1, 5, [3], [0, 1, 3, 7, 19], [19]])
def test_first_step_lands_on_x0(steps, eta):
    tab = ddim_table(_abar64("cosine", 20), steps, eta)
    assert tab["coef_x0"][0] == 1.0 and tab["coef_xt"][0] == 0.0 and tab["sigma"][0] == 0.0
    packed = _engine.pack_sampler_steps(tab)
    assert packed.dtype.itemsize == C.sizeof(_engine.DadSamplerCoef) == 32
    assert packed["coef_x0"][0] == 1.0 and packed["coef_xt"][0] == 0.0 and packed["sigma"][0] == 0.0
    for k in _engine.SAMPLER_COEF_FIELDS:                   # one rounding, of the float64 value
        assert np.array_equal(packed[k], tab[k].astype(np.float32))
    if eta == 0.0:
        assert not tab["sigma"].any()
    elif len(tab["tau"]) > 1:
        assert (tab["sigma"][1:] > 0).all()
    # the mean is sqrt(ap) x0 + sqrt(1 - ap - sigma^2) eps with eps = (x_t - sqrt(ab) x0) / sqrt(1 - ab)
    abar = _abar64("cosine", 20)
    ab = abar[tab["tau"]]
    ap = np.concatenate([np.ones(1), ab[:-1]])
    x0, xt = 0.37, -1.9
    textbook = np.sqrt(ap) * x0 + np.sqrt(np.maximum(1 - ap - tab["sigma"] ** 2, 0)) * (xt - np.sqrt(ab) * x0) / np.sqrt(1 - ab)
    assert np.abs(tab["coef_x0"] * x0 + tab["coef_xt"] * xt - textbook).max() <= 1e-14


def _diffusion(T=20):
    unet = TemporalUnet(6, dim=32, dim_mults=(1, 2))
    return GaussianDiffusion(unet, 8, 4, 2, n_timesteps=T)


def test_every_refusal():
    abar = _abar64("cosine", 20)
    diff = _diffusion()
    bad_steps = [0, -1, 21, [], [3, 2], [0, 4, 4], [0, 20], [-1, 3], [1.5, 2], True]
    for steps in bad_steps:
        with pytest.raises(ValueError):
            ddim_table(abar, steps, 0.0)
        with pytest.raises(ValueError):
            diff.set_sampler("ddim", steps=steps)
    for eta in (-0.1, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            ddim_table(abar, 5, eta)
        with pytest.raises(ValueError):
            diff.set_sampler("ddim", steps=5, eta=eta)
    with pytest.raises(ValueError):
        diff.set_sampler("ddim")                               # no steps
    with pytest.raises(ValueError):
        diff.set_sampler("ddpm", steps=5)
    with pytest.raises(ValueError):
        diff.set_sampler("ddpm", eta=0.5)
    with pytest.raises(ValueError):
        diff.set_sampler("plms", steps=5)
    assert diff.sampler == ("ddpm", None, 0.0) and diff.sampler_plan() is None      # a refusal changes nothing
    # K spans the trained schedule whatever n_timesteps was lowered to
    diff.n_timesteps = 10
    diff.set_sampler("ddim", steps=20, eta=1.0)
    assert diff.sampler == ("ddim", tuple(range(20)), 1.0)
    diff.set_sampler("ddim", steps=[0, 1, 3, 7, 19])
    steps, taus, eta = diff.sampler_plan()
    assert taus == [19, 7, 3, 1, 0] and eta == 0.0 and steps["t"].tolist() == taus       # execution order
    assert steps["coef_x0"][-1] == 1.0 and not steps["sigma"].any()
    diff.set_sampler("ddpm")
    assert diff.sampler == ("ddpm", None, 0.0)


def test_the_sampler_is_plain_data():
    diff = _diffusion()
    keys = list(diff.state_dict().keys())
    diff.set_sampler("ddim", steps=[0, 1, 3, 7, 19], eta=0.5)
    assert list(diff.state_dict().keys()) == keys
    want = ("ddim", (0, 1, 3, 7, 19), 0.5)
    assert diff.sampler == want
    assert copy.deepcopy(diff).sampler == want
    back = pickle.loads(pickle.dumps(diff))
    assert back.sampler == want and list(back.state_dict().keys()) == keys
    a, b = diff.sampler_plan(), back.sampler_plan()
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    fresh = _diffusion()
    fresh.load_state_dict(diff.state_dict())                  # a checkpoint does not carry it
    assert fresh.sampler == ("ddpm", None, 0.0)


# ------------------------------------------------------------------------------------------------ the C entry points
def _one(**kw):
    s = _engine.pack_sampler_steps(ddim_table(_abar64("cosine", census.T), [0, 4, 9]))[1:2].copy()
    for k, v in kw.items():
        s[k] = v
    return s


def test_entry_points_refuse_bad_steps_before_anything_else():
    """A created model: no weights, no schedule, not finalised, no device.  What comes from outside is checked first,
    with the library's codes; a good step then gets as far as 'not finalised'."""
    eng = census.host_engine(6, 32, (1,), 8, 5, "fp32")
    lib = eng.lib
    args = _engine.DadStepArgs()

    def step(s):
        return lib.dad_sampler_step(eng._h, None, s.ctypes.data, 1, C.byref(args), 0, None, 0, None)

    def loop(s, n=None):
        return lib.dad_sampler_loop(eng._h, None, s.ctypes.data, len(s) if n is None else n, 1, None, 0, 0, None, 0, None,
                                    None, 0, None, 0, None)

    good3 = _engine.pack_sampler_steps(ddim_table(_abar64("cosine", census.T), [0, 4, 9]), [2, 1, 0])
    for call in (step, loop):
        assert call(_one(t=census.T)) == DAD_E_RANGE and b"out of bounds" in lib.dad_last_error()
        assert call(_one(t=-1)) == DAD_E_RANGE
        for k in _engine.SAMPLER_COEF_FIELDS:
            assert call(_one(**{k: float("nan")})) == DAD_E_INVALID, k
            assert call(_one(**{k: float("inf")})) == DAD_E_INVALID, k
        assert call(_one(sigma=-0.25)) == DAD_E_INVALID and b"sigma" in lib.dad_last_error()
        assert call(_one()) == DAD_E_STATE                                   # the step itself is fine
    assert loop(good3, 0) == DAD_E_INVALID and b"n_steps" in lib.dad_last_error()
    assert loop(good3, -2) == DAD_E_INVALID
    assert loop(good3) == DAD_E_STATE
    bad_last = good3.copy()
    bad_last["coef_xt"][2] = float("nan")
    assert loop(bad_last) == DAD_E_INVALID and b"step 2" in lib.dad_last_error()
    assert lib.dad_sampler_step(None, None, _one().ctypes.data, 1, C.byref(args), 0, None, 0, None) == DAD_E_INVALID
    assert lib.dad_sampler_step(eng._h, None, None, 1, C.byref(args), 0, None, 0, None) == DAD_E_INVALID
    # the engine's wrappers take the packed dtype only
    with pytest.raises(TypeError):
        eng.sampler_loop(torch.zeros(1, 8, 6), np.zeros(3, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ sanitizers
def test_sampler_host_logic_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "sampler_check"
    src = os.path.join(ROOT, "tests", "sanitize", "sampler_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "sampler host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
