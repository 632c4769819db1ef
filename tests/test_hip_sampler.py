"""The strided (DDIM) sampler on the GPU: dad_sampler_step / dad_sampler_loop and what drives them.

The definitions, restated here on ``oracle.denoiser.unet_forward`` (``restated_loop``).  T = len(betas); abar = the
model's alphas_cumprod as float64; a sampler is strictly ascending tau_0 < ... < tau_{K-1} in [0, T) and eta in [0, 1];
steps = K means tau_i = floor(i T / K).  Step i uses ab = abar[tau_i], ap = abar[tau_{i-1}] (1 for i = 0) and, computed
in float64 and rounded once to fp32,
    sigma = eta sqrt((1 - ap) / (1 - ab)) sqrt(1 - ab / ap),  c = sqrt(max(1 - ap - sigma^2, 0)) / sqrt(1 - ab),
    coef_xt = c,  coef_x0 = sqrt(ap) - c sqrt(ab),  c_recip = sqrt(1 / ab),  c_recipm1 = sqrt(1 / ab - 1),
    guide_x0 = (1 - ab) / sqrt(ab),  guide_mean = 0.
One step: x0 = c_recip x_t - c_recipm1 out (or out); with a guide gradient g, x0 += guide_weight guide_x0 g; clamp;
mean = coef_x0 x0 + coef_xt x_t; x = mean + sigma z; inpaint horizon step 0.  The loop runs i = K-1 .. 0 from x_T;
iteration j evaluates the network at tau_{K-1-j} and uses z_j (Philox draw j + 1).

1. loops against the restatement in float64, by the criterion of tests/test_hip_parity.py: HIP no farther from float64
   than twice the fp32 restatement on the CPU, + 5e-7 — on final_cc_kernel (batch 3, option cc on), on the seam
   (conv_seam_f32, and final_posterior_kernel behind the last step), on final_posterior_kernel alone (step_seam off) and
   on a zero-padded horizon (H = 24: final_posterior_kernel, the seam refuses it);
2. bits: seam on / off, graph replay, second calls, two samplers on one engine, Philox row offsets, eta = 0 draws nothing;
3. the guided step on both tail kernels against a forward error bound built as posterior_reference of
   tests/test_hip_sampling_tail.py builds its own, with the operations of the x0 shift added;
4. the policies: sample_loop / get_actions against the engine-level loop, a value-guided and a projected loop against the
   restatement, and the ancestral sampler's bits after switching back.
"""
import functools

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_hip_parity import dev, injected_noise  # noqa: F401  (dev: fixture)
from tests.test_hip_sampling_tail import CC, POST, U, _ratio
from tests.util import as_torch

T = 20
K5 = 5
IRREGULAR = (0, 1, 3, 7, 19)            # includes T - 1, where the cosine schedule's gain is in the hundreds
ETAS = (0.0, 0.5, 1.0)
# (id, dim, mults, horizon, batch, options, tail kernel of the last step, seam taken, the seam's reason)
TAILS = [
    ("cc_d64_m12_H16_B3", 64, (1, 2), 16, 3, {"cc": 1}, CC, False, "small-batch kernels"),
    ("seam_d128_m1_H32_B3", 128, (1,), 32, 3, {"cc": 0}, POST, True, "taken"),
    ("post_d32_m1_H8_B5", 32, (1,), 8, 5, {"cc": 0, "step_seam": 0}, POST, False, "option off"),
    ("padded_d32_m1_H24_B3", 32, (1,), 24, 3, {"cc": 0}, POST, False, "zero-padded net"),
]
# the first net of tests/test_hip_seam.py on the seam (the third row above switches it off)
SEAM_D32 = ("seam_d32_m1_H8_B5", 32, (1,), 8, 5, {"cc": 0}, POST, True, "taken")
SEAM_D128 = TAILS[1]
TD, OD, AD = 6, 4, 2
# Seeds of the synthetic weights and inputs, and the weights' gain.  Chosen on the CPU restatement so that every clipped
# loop below ends with at least 10 % of its elements strictly inside the clamp (14 - 18 % at the worst combination of
# each net; at gain 1 the eps-predicting nets leave 4 - 8 % at eta = 0, whatever the seed) — and so that no element of a
# clipped eps-predicting loop sits at the clamp's edge behind the step at tau = 19 (EDGE_GAIN, below).
WEIGHT_SEED, INPUT_SEED, GAIN = 55, 96, 2.0
# The criterion compares two fp32 evaluations' distances from float64 and allows a factor of two between them.  That
# presumes both are maxima over many elements.  At tau = 19 of the T = 20 cosine schedule c_recipm1 is 1284: the step
# turns the network's fp32 rounding (up to 1e-6) into 1e-3 of x0.  The clamp then erases that error on every element
# it saturates and keeps it on those it leaves inside; with one or two elements left inside, a clipped loop's whole
# distance is 1284 x ONE element's network rounding, which differs tenfold between two correct fp32 evaluations (two
# CPUs running the fp32 restatement of one such loop: 2.8e-4 and 2.9e-5) — the factor of two then decides by chance.
# So the inputs are chosen, on the float64 truth alone, such that behind every step of gain >= EDGE_GAIN in a clipped
# eps-predicting loop every x0 is outside [-EDGE, EDGE]: all of them saturate, in any evaluation whose x0 is within 0.5
# of the truth (1284 x 5e-6, the project's single-step tolerance, is 6.4e-3).  The unclipped loops keep the gain on every
# element: they are the arithmetic gate.  The test asserts the property.
EDGE_GAIN, EDGE = 100.0, 1.5


# ------------------------------------------------------------------------------------------------ the restatement
def sampler_coefficients(abar64, steps, eta):
    """The definitions of the module docstring; fp32 values (as float64 numbers), index i."""
    T_ = len(abar64)
    tau = np.asarray([(i * T_) // steps for i in range(steps)] if isinstance(steps, int) else list(steps), dtype=np.int64)
    ab = abar64[tau]
    ap = np.concatenate([[1.0], ab[:-1]])
    sigma = eta * np.sqrt((1 - ap) / (1 - ab)) * np.sqrt(1 - ab / ap)
    c = np.sqrt(np.maximum(1 - ap - sigma ** 2, 0.0)) / np.sqrt(1 - ab)
    tab = {"coef_xt": c, "coef_x0": np.sqrt(ap) - c * np.sqrt(ab), "c_recip": np.sqrt(1 / ab),
           "c_recipm1": np.sqrt(1 / ab - 1), "guide_x0": (1 - ab) / np.sqrt(ab), "sigma": sigma}
    return tau, {k: v.astype(np.float32).astype(np.float64) for k, v in tab.items()}


def restated_loop(w, abar64, steps, eta, noise, dtype, predict_epsilon, clip_denoised, cond=None, rest=None,
                  guide_fn=None, guide_weight=0.0, post_step=None, info=None):
    """x after the K steps from x_T = noise[0] with z_j = noise[1 + j], and the last step's x0 before the clamp.
    ``w``: weights of dtype ``dtype``; cond: inpainting of horizon step 0; rest: {k: value} for other horizon steps;
    guide_fn(x, t) -> (B,) score, differentiated at x_t in ``dtype``; post_step(x, tau) after a step; info (a dict)
    receives "edge": the least |x0| before the clamp over the steps with c_recipm1 >= EDGE_GAIN (inf without one)."""
    from oracle import denoiser as orc
    tau, co = sampler_coefficients(abar64, steps, eta)
    K = len(tau)
    f = lambda name, i: torch.tensor(co[name][i], dtype=dtype)
    x = noise[0].to(dtype).clone()
    if cond is not None:
        x[:, 0] = cond.to(dtype)
    for k, v in (rest or {}).items():
        x[:, k] = v.to(dtype)
    x0_pre = None
    for j in range(K):
        i = K - 1 - j
        t = torch.full((x.shape[0],), int(tau[i]), dtype=torch.long)
        g = orc.guide_gradient(guide_fn, x, t) if guide_fn is not None else None
        with torch.no_grad():
            out = orc.unet_forward(w, x, t)
            x0 = f("c_recip", i) * x - f("c_recipm1", i) * out if predict_epsilon else out
            if g is not None:
                x0 = x0 + (torch.tensor(np.float32(guide_weight).item(), dtype=dtype) * f("guide_x0", i)) * g
            x0_pre = x0
            if info is not None and predict_epsilon and co["c_recipm1"][i] >= EDGE_GAIN:
                info["edge"] = min(info.get("edge", float("inf")), float(x0.abs().min()))
            if clip_denoised:
                x0 = torch.clamp(x0, -1.0, 1.0)
            x = f("coef_x0", i) * x0 + f("coef_xt", i) * x + f("sigma", i) * noise[1 + j].to(dtype)
            if cond is not None:
                x[:, 0] = cond.to(dtype)
            for k, v in (rest or {}).items():
                x[:, k] = v.to(dtype)
            if post_step is not None:
                x = post_step(x, int(tau[i]))
    return x, x0_pre


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Weights (fp32 and float64), x_T and z stack, conditions of a tail's net; nobody writes into them."""
    from dynamics_aware_diffusion_amd.models.diffusion import make_schedule
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    _, dim, mults, H, B = next(n for n in TAILS + [SEAM_D32] if n[0] == name)[:5]
    state = synth.synth_unet_state(TD, dim, mults, seed=WEIGHT_SEED, affine_jitter=0.3, gain=GAIN)
    w32 = as_torch(state)
    return {"state": state, "w32": w32, "w64": orc.cast_weights(w32, torch.float64),
            "noise": torch.from_numpy(synth.normal_like(INPUT_SEED, f"sampler.noise.{name}", (K5 + 1, B, H, TD))),
            "cond": torch.from_numpy(synth.uniform(INPUT_SEED, f"sampler.cond.{name}", (B, TD), 0.9)),
            "abar": make_schedule("cosine", T)["alphas_cumprod"].to(torch.float64).numpy()}


@functools.lru_cache(maxsize=None)
def _reference(name, steps, eta, pe, clip, cond_mode):
    """(float64 truth, fp32 restatement, the truth's last x0 before the clamp, the truth's least |x0| behind a step of
    gain >= EDGE_GAIN) of one loop; computed once."""
    inp = _inputs(name)
    cond = {"none": None, "shared": inp["cond"][:1], "rows": inp["cond"]}[cond_mode]
    info = {}
    x64, pre64 = restated_loop(inp["w64"], inp["abar"], steps, eta, inp["noise"], torch.float64, pe, clip, cond, info=info)
    x32, _ = restated_loop(inp["w32"], inp["abar"], steps, eta, inp["noise"], torch.float32, pe, clip, cond)
    return x64, x32, pre64, info.get("edge", float("inf"))


def _diffusion(tail, dev, pe=True, clip=True):
    from tests.test_hip_long_horizon import _diffusion as build
    name, dim, mults, H, B, options, kernel, taken, reason = tail
    diff = build(TD, OD, AD, dim, mults, H, T, _inputs(name)["state"], dev, predict_epsilon=bool(pe), clip_denoised=bool(clip))
    eng = diff._engine(dev)
    for k, v in options.items():
        eng.debug_set_option(k, v)
    q = eng.seam_plan(B)
    assert eng.forward_plan(B, 0)["final"][2] == kernel, (name, eng.forward_plan(B, 0)["final"])
    assert q["taken"] == taken and q["reason"] == reason, (name, q)
    return diff, eng


def _steps(diff, steps, eta):
    """The engine's array in execution order, through the public switch."""
    diff.set_sampler("ddim", steps=list(steps) if not isinstance(steps, int) else steps, eta=eta)
    return diff.sampler_plan()[0]


def _loop(eng, steps, inp, dev, cond_mode="none", noise_mode="injected", seed=0x123456789ABCDEF, row_offset=0,
          stack=None, **kw):
    x = inp["noise"][0].to(dev).clone()
    cond = {"none": None, "shared": inp["cond"][:1], "rows": inp["cond"]}[cond_mode]
    if cond is not None:
        cond = cond.to(dev).contiguous()
        x[:, 0] = cond
    if noise_mode == "injected":
        stack = inp["noise"][1:1 + len(steps)] if stack is None else stack
        eng.sampler_loop(x, steps, noise_stack=stack.to(dev).contiguous(), cond0=cond, **kw)
    else:
        eng.sampler_loop(x, steps, seed=seed, row_offset=row_offset, cond0=cond, **kw)
    torch.cuda.synchronize()
    return x.cpu()


def _gate(got, x64, x32, what, misses=None):
    """The criterion; with ``misses`` a miss is recorded there (and asserted by the caller, after every figure is out)."""
    d_hip = float((got.double() - x64).abs().max())
    d_32 = float((x32.double() - x64).abs().max())
    ok = bool(np.isfinite(d_hip) and d_hip <= 2 * d_32 + 5e-7)
    print(f"{what}: |hip - f64| = {d_hip:.3e}   |fp32 restatement - f64| = {d_32:.3e}   max |x| = {float(x64.abs().max()):.2f}"
          f"{'' if ok else '   MISSES THE GATE'}")
    if misses is None:
        assert ok, what
    elif not ok:
        misses.append(f"{what}: {d_hip:.3e} > 2 x {d_32:.3e} + 5e-7")
    return d_hip, d_32


# ------------------------------------------------------------------------------------------------ 1. loops vs float64
@pytest.mark.gpu
@pytest.mark.parametrize("clip", (0, 1))
@pytest.mark.parametrize("pe", (0, 1))
@pytest.mark.parametrize("tail", TAILS, ids=lambda n: n[0])
def test_strided_loop_vs_float64(tail, pe, clip, dev):
    """Every loop of the matrix against the criterion; each prints both distances, and the misses are asserted after all
    figures are out.  With inputs that left one element of 576 inside the clamp behind the step at tau = 19 (see EDGE_GAIN
    above) the seam net's clipped eps-predicting loops without a condition were 5.3e-4 / 4.2e-5 / 1.2e-4 (eta 0 / 0.5 / 1)
    from float64 on the MI355X where the fp32 restatement on that machine's CPU was 2.9e-5 / 2.2e-6 / 6.2e-6 and on
    another CPU 2.8e-4: one element's rounding times 1284 on either side."""
    name = tail[0]
    misses = []
    inp = _inputs(name)
    diff, eng = _diffusion(tail, dev, pe, clip)
    print()
    for steps in (K5, IRREGULAR):
        for eta in ETAS:
            arr = _steps(diff, steps, eta)
            for cond_mode in ("none", "shared", "rows"):
                x64, x32, pre64, edge = _reference(name, steps, eta, pe, clip, cond_mode)
                got = _loop(eng, arr, inp, dev, cond_mode)
                what = f"{name} pe={pe} clip={clip} steps={steps} eta={eta} cond={cond_mode}"
                _gate(got, x64, x32, what, misses)
                if not clip:
                    continue
                free = slice(1, None) if cond_mode != "none" else slice(None)          # (inpainted rows are copies)
                inside = float((x64[:, free].abs() < 1.0).double().mean())
                print(f"    {100 * inside:.0f} % of the compared elements inside (-1, 1); least |x0| behind a step of gain >= "
                      f"{EDGE_GAIN:.0f}: {edge:.2f}")
                assert inside >= 0.10, what
                assert edge > EDGE, what
                # the last step is x = clamp(x0): nothing leaves [-1, 1], and what the truth saturates by more than
                # 1e-4 — many times the loop's error — is exactly +-1
                assert float(got.abs().max()) <= 1.0, what
                far = pre64[:, free].abs() > 1.0 + 1e-4
                assert torch.equal(got[:, free][far].double(), torch.sign(pre64[:, free][far])), what
    assert diff.model._engine is eng, "setting the sampler rebuilt the engine"
    assert not misses, misses


# ------------------------------------------------------------------------------------------------ 2. bits
@pytest.mark.gpu
@pytest.mark.parametrize("tail", [SEAM_D128, SEAM_D32], ids=lambda n: n[0])
def test_seam_on_is_bit_equal_to_seam_off(tail, dev):
    inp = _inputs(tail[0])
    for pe, clip in ((1, 1), (0, 0)):
        diff, eng = _diffusion(tail, dev, pe, clip)
        try:
            for steps in (1, 2, K5, IRREGULAR):
                for eta in (0.0, 0.5):
                    arr = _steps(diff, steps, eta)
                    for noise_mode in ("injected", "philox"):
                        for cond_mode in ("none", "rows"):
                            got = {}
                            for on in (1, 0):
                                eng.debug_set_option("step_seam", on)
                                assert eng.seam_plan(tail[4])["taken"] == bool(on)
                                got[on] = _loop(eng, arr, inp, dev, cond_mode, noise_mode)
                            assert torch.isfinite(got[1]).all()
                            assert torch.equal(got[1], got[0]), (tail[0], pe, clip, steps, eta, noise_mode, cond_mode)
        finally:
            eng.debug_set_option("step_seam", 1)


def _graph_loop(eng, arr, inp, dev, noise_mode, seed=7):
    """A loop on address-stable buffers, as a replayed graph needs them."""
    B, H = inp["noise"].shape[1:3]
    x = eng.persistent("test.x", (B, H, TD)).copy_(inp["noise"][0].to(dev))
    cond = eng.persistent("test.cond", (1, TD)).copy_(inp["cond"][:1].to(dev))
    x[:, 0] = cond
    if noise_mode == "injected":
        z = eng.persistent("test.z", (len(arr), B, H, TD)).copy_(inp["noise"][1:1 + len(arr)].to(dev))
        eng.sampler_loop(x, arr, noise_stack=z, cond0=cond, use_graph=True)
    else:
        eng.sampler_loop(x, arr, seed=seed, cond0=cond, use_graph=True)
    torch.cuda.synchronize()
    return x.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("tail", TAILS[:3], ids=lambda n: n[0])
def test_second_call_and_graph_replay_give_the_same_bits(tail, dev):
    inp = _inputs(tail[0])
    diff, eng = _diffusion(tail, dev)
    a = _steps(diff, K5, 0.5)
    b = _steps(diff, IRREGULAR, 0.5)
    for noise_mode in ("injected", "philox"):
        kw = dict(noise_mode=noise_mode, seed=7)
        first = _loop(eng, a, inp, dev, "shared", **kw)
        assert torch.equal(first, _loop(eng, a, inp, dev, "shared", **kw)), "a second call gives other bits"
        graph = _graph_loop(eng, a, inp, dev, noise_mode)
        assert torch.equal(first, graph), "graph replay differs from eager"
        assert torch.equal(graph, _graph_loop(eng, a, inp, dev, noise_mode)), "a second replay gives other bits"
        # a second sampler on the same buffers: captured on its own, and the first one's graph is still the first one's
        other = _graph_loop(eng, b, inp, dev, noise_mode)
        assert torch.equal(other, _loop(eng, b, inp, dev, "shared", **kw)), "the second sampler replays something else"
        assert not torch.equal(other, graph)
        assert torch.equal(graph, _graph_loop(eng, a, inp, dev, noise_mode)), "switching back replays another result"
        assert torch.equal(other, _graph_loop(eng, b, inp, dev, noise_mode))


@pytest.mark.gpu
def test_philox_rows_do_not_depend_on_the_sharding(dev):
    inp = _inputs(SEAM_D32[0])
    diff, eng = _diffusion(SEAM_D32, dev)
    arr = _steps(diff, K5, 1.0)
    seed, base, r0, r1 = 0xFEDCBA987654321, 2 ** 27 + 3, 1, 4
    assert eng.seam_plan(r1 - r0)["taken"] and eng.forward_plan(r1 - r0, 0)["final"][2] == POST

    def run(rows, offset):
        x = torch.empty(len(rows), inp["noise"].shape[2], TD, device=dev)
        eng.fill_normal(x, seed, row_offset=offset, draw=0)
        cond = inp["cond"][rows].to(dev).contiguous()
        x[:, 0] = cond
        eng.sampler_loop(x, arr, seed=seed, row_offset=offset, cond0=cond)
        torch.cuda.synchronize()
        return x.cpu()

    whole = run(list(range(5)), base)
    part = run(list(range(r0, r1)), base + r0)
    assert torch.isfinite(whole).all() and torch.equal(whole[r0:r1], part)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", TAILS[:3], ids=lambda n: n[0])
def test_eta_zero_draws_nothing(tail, dev):
    from dynamics_aware_diffusion_amd.utils import synth
    inp = _inputs(tail[0])
    diff, eng = _diffusion(tail, dev)
    arr = _steps(diff, K5, 0.0)
    assert not arr["sigma"].any()
    B, H = inp["noise"].shape[1:3]
    # values, not bits: 0 * z is -0 or +0 by the sign of z
    want = _loop(eng, arr, inp, dev, "shared")
    other = torch.from_numpy(synth.normal_like(61, "sampler.other", (K5, B, H, TD)))
    assert torch.all(_loop(eng, arr, inp, dev, "shared", stack=other) == want)
    assert torch.all(_loop(eng, arr, inp, dev, "shared", "philox", seed=1) == want)
    assert torch.all(_loop(eng, arr, inp, dev, "shared", "philox", seed=2 ** 63 + 5) == want)
    # the torch route: one randn, for x_T — the harness holds one tensor and fails on a second request
    from dynamics_aware_diffusion_amd import GuidedPolicy
    assert diff.sampler_rng == "torch"
    with injected_noise(inp["noise"][:1].numpy(), dev):
        x = diff.p_sample_loop((B, H, TD))
    torch.cuda.synchronize()
    assert torch.all(x.cpu() == _loop(eng, arr, inp, dev, "none"))
    pol = GuidedPolicy(diff, None)
    with injected_noise(inp["noise"][:1].numpy(), dev):
        x = pol.sample_loop(batch_size=B, conditions={0: inp["cond"][:1].to(dev)})
    torch.cuda.synchronize()
    assert torch.all(x.cpu() == want)
    # eta > 0 asks for K more, in loop order
    diff.set_sampler("ddim", steps=K5, eta=0.5)
    with injected_noise(inp["noise"].numpy(), dev):
        x = pol.sample_loop(batch_size=B, conditions={0: inp["cond"][:1].to(dev)})
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), _loop(eng, diff.sampler_plan()[0], inp, dev, "shared"))
    diff.max_noise_stack_bytes = 0                  # z per step: the same draws in the same order, the same bits here
    with injected_noise(inp["noise"].numpy(), dev):
        y = pol.sample_loop(batch_size=B, conditions={0: inp["cond"][:1].to(dev)})
    with injected_noise(inp["noise"].numpy(), dev):
        y2 = diff.p_sample_loop((B, H, TD))
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), x.cpu())
    assert torch.equal(y2.cpu(), _loop(eng, diff.sampler_plan()[0], inp, dev, "none"))
    assert diff.model._engine is eng


# ------------------------------------------------------------------------------------------------ 3. the guided step
GUIDE_WEIGHT = 0.7
STEP_NETS = {CC: 3, POST: 70}           # batch of the tiny net (td 6, dim 32, one level, H 8) per tail kernel


@functools.lru_cache(maxsize=None)
def _step_inputs(B):
    from dynamics_aware_diffusion_amd.utils import synth
    shape = (B, 8, TD)
    return tuple(synth.normal_like(67, f"sampler.step.{k}.{B}", shape) for k in "xzg") + \
        (synth.uniform(67, f"sampler.step.c.{B}", (B, TD), 0.9),)


def guided_step_reference(co, x, eps, z, g, guide_weight, cond, predict_epsilon, clip_denoised):
    """One step of the module docstring in float64 on a given network output, and the forward error bound of the tail
    kernels' evaluation of it, built as posterior_reference (tests/test_hip_sampling_tail.py): every rounded fp32
    operation contributes u |its exact result|, errors already made travel on, an fma counts as its mul and its add.
        a = c_recip x, b = c_recipm1 eps, x0 = a - b      u (|a| + |b| + |x0|)          [predict_epsilon; else exact]
        gx = weight guide_x0 (host), q = gx g, x0 += q    2 u |q| + u |x0|: the two products and the sum
        clamp                                             1-Lipschitz
        c = coef_x0 x0, d = coef_xt x, mean = c + d       |coef_x0| e(x0) + u (|c| + |d| + |mean|)
        weight guide_mean g with guide_mean = 0           adds an exact 0
        s = sigma z, x = mean + s                         e(mean) + u |s| + u |x|   (sigma is data: no expf here)
    Inpainted rows are copies: bound 0.  Returns (mean, x, bound of mean_out, bound of x, x0 inside the clamp)."""
    u = U / (1.0 - 16.0 * U)
    if predict_epsilon:
        a, b = co["c_recip"] * x, co["c_recipm1"] * eps
        x0 = a - b
        e0 = u * (np.abs(a) + np.abs(b) + np.abs(x0))
    else:
        x0, e0 = eps.copy(), np.zeros_like(eps)
    q = (float(np.float32(guide_weight)) * co["guide_x0"]) * g
    x0 = x0 + q
    e0 = e0 + 2.0 * u * np.abs(q) + u * np.abs(x0)
    inside = int((np.abs(x0) < 1.0).sum())
    if clip_denoised:
        x0 = np.clip(x0, -1.0, 1.0)
    c, d = co["coef_x0"] * x0, co["coef_xt"] * x
    mean = c + d
    em = abs(co["coef_x0"]) * e0 + u * (np.abs(c) + np.abs(d) + np.abs(mean))
    s = co["sigma"] * z
    xn = mean + s
    ex = em + u * np.abs(s) + u * np.abs(xn)
    xn[:, 0], ex[:, 0] = cond, 0.0
    return mean, xn, em, ex, inside


@pytest.mark.gpu
@pytest.mark.parametrize("clip", (0, 1))
@pytest.mark.parametrize("pe", (0, 1))
@pytest.mark.parametrize("kernel", (CC, POST))
def test_guided_step_vs_float64_bound(kernel, pe, clip, dev):
    from tests.test_hip_long_horizon import _diffusion as build
    from tests.test_hip_sampling_tail import _net
    B = STEP_NETS[kernel]
    diff = build(TD, TD - 1, 1, 32, (1,), 8, T, _net(TD, 32, True), dev, predict_epsilon=bool(pe), clip_denoised=bool(clip))
    eng = diff._engine(dev)
    assert eng.forward_plan(B, 0)["final"][2] == kernel
    x_h, z_h, g_h, cond_h = _step_inputs(B)
    x, z, g, cond = (torch.from_numpy(v).to(dev) for v in (x_h, z_h, g_h, cond_h))
    arr = _steps(diff, IRREGULAR, 0.5)               # execution order: tau = 19, 7, 3, 1, 0
    worst = 0.0
    print()
    for j in (2, len(arr) - 1):                      # a middle step (tau = 3) and i = 0
        co = {k: float(arr[k][j]) for k in arr.dtype.names[1:]}
        assert (co["sigma"] > 0) == (j == 2) and co["guide_x0"] > 0 and co["guide_mean"] == 0.0

        def step(**over):
            xs, mean, eps = x.clone(), torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
            eng.sampler_step(xs, arr[j], **{**dict(noise=z, cond0=cond, guide_grad=g, guide_weight=GUIDE_WEIGHT), **over},
                             mean_out=mean, eps_out=eps)
            torch.cuda.synchronize()
            return xs.cpu().numpy(), mean.cpu().numpy(), eps.cpu().numpy()

        xa, mean_a, eps_a = step()
        xb, mean_b, eps_b = step()
        assert np.array_equal(xa, xb) and np.array_equal(mean_a, mean_b) and np.array_equal(eps_a, eps_b)
        x0g, mean_0g, _ = step(guide_grad=None, guide_weight=0.0)
        xw0, mean_w0, _ = step(guide_weight=0.0)
        assert np.array_equal(xw0, x0g) and np.array_equal(mean_w0, mean_0g), "a guide gradient of weight 0 changed bits"
        assert not np.array_equal(mean_a, mean_0g), "the guide moved nothing"
        assert np.isfinite(xa).all() and np.isfinite(mean_a).all() and np.isfinite(eps_a).all()
        assert np.array_equal(xa[:, 0], cond_h)
        if j == len(arr) - 1:
            assert np.array_equal(xa[:, 1:], mean_a[:, 1:]), "i == 0: x is not mean_out"
        mean64, xn64, em, ex, inside = guided_step_reference(
            co, x_h.astype(np.float64), eps_a.astype(np.float64), z_h.astype(np.float64), g_h.astype(np.float64),
            GUIDE_WEIGHT, cond_h.astype(np.float64), pe, clip)
        r_mean, r_x = _ratio(np.abs(mean_a - mean64), em), _ratio(np.abs(xa - xn64), ex)
        print(f"{kernel} pe={pe} clip={clip} tau={int(arr['t'][j])}: error / bound of mean_out {r_mean:.3f}, of x {r_x:.3f}; "
              f"{inside} of {xa.size} x0 inside the clamp")
        worst = max(worst, r_mean, r_x)
        if clip:
            assert 0 < inside < xa.size, "the inputs do not straddle the clamp"
    print(f"worst error / bound: {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the policies
def _policy_setup(dev, pe=True, clip=True):
    diff, eng = _diffusion(SEAM_D32, dev, pe, clip)
    return diff, eng, _inputs(SEAM_D32[0])


@pytest.mark.gpu
def test_policy_loops_are_the_engine_level_loop(dev):
    from dynamics_aware_diffusion_amd import GuidedPolicy
    diff, eng, inp = _policy_setup(dev)
    B, H = inp["noise"].shape[1:3]
    before = None
    pol = GuidedPolicy(diff, cases.NormalizerStub(OD, AD), action_horizon=2)
    cond0, cond3 = inp["cond"][:1].to(dev), inp["cond"][1:2].to(dev)
    with injected_noise(inp["noise"].numpy(), dev):                # the ancestral loop, before any sampler is set
        diff.n_timesteps = K5
        before = pol.sample_loop(batch_size=B, conditions={0: cond0}).cpu()
        diff.n_timesteps = T
    diff.set_sampler("ddim", steps=K5, eta=0.5)
    arr, taus, _ = diff.sampler_plan()
    # a condition at horizon step 0: the fused loop
    with injected_noise(inp["noise"].numpy(), dev):
        got = pol.sample_loop(batch_size=B, conditions={0: cond0})
    assert torch.equal(got.cpu(), _loop(eng, arr, inp, dev, "shared"))
    # ... and at another step: one engine step per iteration
    with injected_noise(inp["noise"].numpy(), dev):
        got = pol.sample_loop(batch_size=B, conditions={0: cond0, 3: cond3})
    x = inp["noise"][0].to(dev).clone()
    x[:, 0], x[:, 3] = cond0, cond3
    for j in range(K5):
        eng.sampler_step(x, arr[j], noise=inp["noise"][1 + j].to(dev), cond0=cond0)
        x[:, 3] = cond3
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), x.cpu())
    # get_actions: Philox, per-row conditions, the graph route
    diff.sampler_rng, diff.seed, diff.use_graph = "philox", 0xABCDEF, True
    try:
        obs = inp["cond"][:, :OD].numpy() * 2.0
        acts = pol.get_actions(obs)
        nz = pol.normalizer
        start = torch.zeros(B, TD, device=dev)
        start[:, :OD] = (torch.from_numpy(obs).to(dev) - torch.from_numpy(nz.obs_mean).to(dev)) / torch.from_numpy(nz.obs_std).to(dev)
        x = torch.empty(B, H, TD, device=dev)
        eng.fill_normal(x, diff.seed, draw=0)
        x[:, 0] = start
        eng.sampler_loop(x, arr, seed=diff.seed, cond0=start.contiguous())
        want = (x[:, :3, OD:] * torch.from_numpy(nz.action_std).to(dev) + torch.from_numpy(nz.action_mean).to(dev)).cpu().numpy()
        assert np.array_equal(acts, want[:, 0]) and np.array_equal(pol.get_actions(obs), want[:, 1])
    finally:
        diff.sampler_rng, diff.use_graph = "torch", False
    # back to the ancestral sampler: the bits it gave before any sampler was set
    diff.set_sampler("ddpm")
    with injected_noise(inp["noise"].numpy(), dev):
        diff.n_timesteps = K5
        after = pol.sample_loop(batch_size=B, conditions={0: cond0}).cpu()
        diff.n_timesteps = T
    assert torch.equal(before, after)
    assert diff.model._engine is eng


def _value_fn(dtype):
    vw = {k: v.to(dtype) for k, v in as_torch(cases.value_net_weights(OD)).items()}
    F = torch.nn.functional

    def value(obs):
        return F.linear(torch.tanh(F.linear(obs, vw["w1"].to(obs.device), vw["b1"].to(obs.device))),
                        vw["w2"].to(obs.device), vw["b2"].to(obs.device))
    return value


@pytest.mark.gpu
@pytest.mark.parametrize("pe,clip,eta", [(1, 1, 0.0), (1, 0, 0.5), (0, 1, 1.0)])
def test_value_guided_loop_vs_float64(pe, clip, eta, dev):
    from dynamics_aware_diffusion_amd import ValueGuidedPolicy
    diff, eng, inp = _policy_setup(dev, pe, clip)
    B = inp["noise"].shape[1]
    gw = 0.7

    class V(torch.nn.Module):
        def forward(self, obs):
            return _value_fn(torch.float32)(obs)

    pol = ValueGuidedPolicy(diff, None, V(), guide_weight=gw)
    cond = inp["cond"][:1]
    diff.set_sampler("ddim", steps=list(IRREGULAR), eta=eta)
    with injected_noise(inp["noise"].numpy() if eta > 0 else inp["noise"][:1].numpy(), dev):
        got = pol.sample_loop(batch_size=B, conditions={0: cond.to(dev)}).cpu()
    ref = {}
    for dtype, w in ((torch.float64, inp["w64"]), (torch.float32, inp["w32"])):
        value = _value_fn(dtype)
        ref[dtype], _ = restated_loop(w, inp["abar"], IRREGULAR, eta, inp["noise"], dtype, pe, clip, cond,
                                      guide_fn=lambda x, t: value(x[:, :, :OD]).sum(dim=1), guide_weight=gw)
    unguided, _ = restated_loop(inp["w64"], inp["abar"], IRREGULAR, eta, inp["noise"], torch.float64, pe, clip, cond)
    print()
    _gate(got, ref[torch.float64], ref[torch.float32], f"value-guided pe={pe} clip={clip} eta={eta}")
    moved = float((ref[torch.float64] - unguided).abs().max())
    print(f"    the guide moves the plan by up to {moved:.3f}")
    assert moved > 1e-2, "the guide is too weak for this test to see it"


@pytest.mark.gpu
@pytest.mark.parametrize("sched,eta", [("constant", 0.0), ("linear", 0.5)])
def test_projected_loop_vs_float64(sched, eta, dev):
    from dynamics_aware_diffusion_amd import DynamicsAwarePolicy
    from oracle import projection as oproj
    diff, eng, inp = _policy_setup(dev)
    B, H = inp["noise"].shape[1:3]
    A, Bm = oproj.double_integrator(0.1)
    P = oproj.projection_matrix(A, Bm, H)
    nz = cases.NormalizerStub(OD, AD)
    strength = 0.6
    pol = DynamicsAwarePolicy(diff, projection_matrix=P, normalizer=nz, state_dim=OD, observation_dim=OD, action_dim=AD,
                              horizon=H, projection_schedule=sched, projection_strength=strength,
                              project_during_sampling=True)
    cond = inp["cond"][:1]
    diff.set_sampler("ddim", steps=K5, eta=eta)
    assert not eng.seam_plan(B, projection=True)["taken"]
    with injected_noise(inp["noise"].numpy() if eta > 0 else inp["noise"][:1].numpy(), dev):
        got = pol.sample_loop(batch_size=B, conditions={0: cond.to(dev)}).cpu()
    ref = {}
    for dtype, w in ((torch.float64, inp["w64"]), (torch.float32, inp["w32"])):
        stats = [torch.from_numpy(v).to(dtype) for v in (nz.obs_mean, nz.obs_std, nz.action_mean, nz.action_std)]
        post = lambda x, tau: oproj.apply_projection(x, P.to(dtype), oproj.projection_alpha(sched, strength, tau, T), OD, OD, *stats)
        ref[dtype], _ = restated_loop(w, inp["abar"], K5, eta, inp["noise"], dtype, True, True, cond, post_step=post)
    plain, _ = restated_loop(inp["w64"], inp["abar"], K5, eta, inp["noise"], torch.float64, True, True, cond)
    print()
    _gate(got, ref[torch.float64], ref[torch.float32], f"projected {sched} eta={eta}")
    assert float((ref[torch.float64] - plain).abs().max()) > 1e-2, "the projection moves nothing"
