"""GPU parity of horizons above 128 positions: layers longer than any whole-sample tile run on windowed tiles
(csrc/conv_gemm.hpp WIN: BN positions of one sample plus a halo read from the neighbouring positions) and their
GroupNorm -> Mish -> time embedding -> residual tail as a pass over whole (sample, group) pairs (csrc/conv_gn_pass.hpp).

Gates as tests/test_hip_parity.py: one forward <= 5e-6 and no farther from the fp64 run than 2x the fp32 reference
(+5e-7); a loop <= 2e-5.  Against the reference's own runs (tests/golden/make_golden_long.py: H = 256 and the padded
H = 200, forward + a conditioned T = 20 loop) in both arithmetics, against the oracle on further nets (H = 512, padded
H = 384, kernel sizes 3 / 7, zero-padded widths at dim 96, batch 1 and 256), plus a full-size property run.
Gradients (loss.backward() through the engine: the windowed data-gradient convs, the windowed weight-gradient kernel,
the GroupNorm backward over pairs of up to C/8 x 512 elements): every parameter and d loss / d x_t <= 2e-5 max|g|
against the reference's own gradients at H = 256 and the oracle's autograd on the nets above; two backward passes
bit-identical."""
import numpy as np
import pytest
import torch

from oracle import denoiser as orc
from tests.golden import cases
from tests.golden.cases_long import LONG_CASES, LONG_GRAD_CASES, long_train_inputs
from tests.test_hip_parity import TOL_LOOP, TOL_STEP, dev, injected_noise  # noqa: F401  (dev: fixture)
from tests.util import as_torch, golden, grad_scales, max_abs

pytestmark = pytest.mark.gpu

REL = 2e-5


def _diffusion(td, od, ad, dim, mults, H, T, state, dev, ks=5, precision="fp32", **kw):
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    unet = TemporalUnet(td, dim=dim, dim_mults=mults, kernel_size=ks)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    unet.precision = precision
    return GaussianDiffusion(unet, H, od, ad, n_timesteps=T, **kw).to(dev)


def _backward(diff, x0, t, noise, loss_type, dev):
    """loss.backward() of diffusion.py:253-290 on given draws with x_t a leaf: (loss, d x_t, parameter gradients)."""
    for p in diff.parameters():
        p.grad = None
    x0t, tt, nz = torch.from_numpy(x0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(noise).to(dev)
    with torch.enable_grad():
        x_t = diff.q_sample(x0t, tt, nz).detach().requires_grad_(True)
        out = diff.model(x_t, tt)
        loss = diff.loss_fn(out, nz).mean()
        loss.backward()
    torch.cuda.synchronize()
    return (float(loss), x_t.grad.cpu().numpy(),
            {k: p.grad.detach().cpu().numpy().copy() for k, p in diff.model.named_parameters()})


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c[0])
def test_long_horizons_vs_reference(case, precision, dev):
    """H = 256 (level 0 at 256 positions: windowed convs of every Conv1dBlock there, the first block's 1x1 residual
    conv from transition_dim, the final Conv1dBlock) and H = 200 (padded to 256: zero rows 200..255 left out of the
    statistics) against the reference; a conditioned loop with injected noise; the inpainted row exact; in-kernel
    Philox sampling deterministic.  Split-f16 nets run the windowed layers in fp32 and their short ones split."""
    from dynamics_aware_diffusion_amd import GuidedPolicy
    name, net, Hz, B, t = case
    g = golden(name)
    od, ad, td, dim, mults = cases.net_dims(net)
    T = cases.NETS[net][4]
    diff = _diffusion(td, od, ad, dim, mults, Hz, T, cases.net_weights(net), dev, precision=precision)
    assert diff._engine(dev).small_batch_plan(B) == (0, 0)
    x, noise = cases.horizon_inputs(name, net, Hz, B, T)
    got = diff.model(torch.from_numpy(x).to(dev), t).cpu().numpy()
    err32, err64, ref64 = max_abs(got, g["eps"]), max_abs(got, g["eps_fp64"]), max_abs(g["eps"], g["eps_fp64"])
    print(f"{name} {precision}: |hip-ref32|={err32:.2e} |hip-fp64|={err64:.2e} |ref32-fp64|={ref64:.2e}")
    assert err32 <= TOL_STEP
    assert err64 <= 2 * ref64 + 5e-7
    pol = GuidedPolicy(diff, None)
    cond = {0: torch.from_numpy(cases.loop_condition(name, net)).to(dev)}
    with injected_noise(noise, dev):
        xf = pol.sample_loop(batch_size=B, conditions=cond)
    torch.cuda.synchronize()
    xf = xf.cpu().numpy()
    assert max_abs(xf, g["x_final"]) <= TOL_LOOP
    assert np.array_equal(xf[:, 0], np.repeat(cond[0].cpu().numpy(), B, 0))
    diff.sampler_rng, diff.seed = "philox", 5
    a = pol.sample_loop(batch_size=B, conditions=cond).cpu().numpy()
    b = pol.sample_loop(batch_size=B, conditions=cond).cpu().numpy()
    assert a.shape == (B, Hz, td) and np.isfinite(a).all() and np.array_equal(a, b)
    assert np.array_equal(a[:, 0], np.repeat(cond[0].cpu().numpy(), B, 0))


# (id, obs_dim, act_dim, dim, mults, horizon, kernel_size, batch)
ORACLE_NETS = [
    ("H512_dim32_148", 4, 2, 32, (1, 4, 8), 512, 5, 2),          # levels 0 and 1 windowed, down / up convs included
    ("H384_dim32_148", 4, 2, 32, (1, 4, 8), 384, 5, 2),          # padded to 512
    ("H256_dim96_124", 4, 2, 96, (1, 2, 4), 256, 5, 2),          # zero-padded GroupNorm groups (96 -> 128)
    ("H256_k3", 4, 2, 32, (1, 2, 4), 256, 3, 3),
    ("H256_k7", 5, 3, 32, (1, 2, 4), 256, 7, 2),
    ("H256_dim64_B1", 4, 2, 64, (1, 2, 4), 256, 5, 1),           # batch 1: grid split-K on windowed tiles
    ("H256_dim32_B256", 4, 2, 32, (1, 2, 4), 256, 5, 256),
    ("H512_k7_dim32_12", 5, 3, 32, (1, 2), 512, 7, 2),           # the decoder's [x | skip] block at 256 positions
]


@pytest.mark.parametrize("net", ORACLE_NETS, ids=lambda n: n[0])
def test_long_horizon_nets_vs_oracle(net, dev):
    from dynamics_aware_diffusion_amd.utils import synth
    name, od, ad, dim, mults, H, ks, B = net
    td = od + ad
    state = synth.synth_unet_state(td, dim, mults, seed=31, kernel_size=ks, affine_jitter=0.25)
    diff = _diffusion(td, od, ad, dim, mults, H, 20, state, dev, ks=ks)
    x = torch.from_numpy(synth.normal_like(71, "long." + name, (B, H, td)))
    t = 13
    got = diff.model(x.to(dev), t)
    again = diff.model(x.to(dev), t)
    torch.cuda.synchronize()
    assert torch.equal(got, again)                     # fixed reduction order across the windowed tiles
    got = got.cpu().numpy()
    w = as_torch(state)
    tt = torch.full((B,), t, dtype=torch.long)
    with torch.no_grad():
        want = orc.unet_forward(w, x, tt).numpy()
        want64 = orc.unet_forward(orc.cast_weights(w, torch.float64), x.double(), tt).numpy()
    err, err64, ref64 = max_abs(got, want), max_abs(got, want64), max_abs(want, want64)
    print(f"{name}: |hip-orc32|={err:.2e} |hip-fp64|={err64:.2e} |orc32-fp64|={ref64:.2e}")
    assert err <= TOL_STEP
    assert err64 <= 2 * ref64 + 5e-7


def test_full_size_property_run(dev):
    """dim 128, mults (1, 2, 4, 8) at H = 256, B = 256: one conditioned T = 100 loop gives finite plans clipped to
    [-1, 1] with the inpainted row exact, deterministic, rows 0..3 equal to a batch-4 run to fp32 rounding."""
    from dynamics_aware_diffusion_amd import GuidedPolicy
    from dynamics_aware_diffusion_amd.utils import synth
    od, ad, dim, mults, H, B, T = 4, 2, 128, (1, 2, 4, 8), 256, 256, 100
    td = od + ad
    state = synth.synth_unet_state(td, dim, mults, seed=32, affine_jitter=0.25)
    diff = _diffusion(td, od, ad, dim, mults, H, T, state, dev)
    diff.sampler_rng, diff.seed = "philox", 99
    pol = GuidedPolicy(diff, None)
    c = synth.uniform(72, "long.full.cond", (1, td), 0.9)
    c[:, od:] = 0.0
    cond = {0: torch.from_numpy(c).to(dev)}
    big = pol.sample_loop(batch_size=B, conditions=cond)
    big2 = pol.sample_loop(batch_size=B, conditions=cond)
    small = pol.sample_loop(batch_size=4, conditions=cond)
    torch.cuda.synchronize()
    assert big.shape == (B, H, td)
    assert torch.equal(big, big2) and torch.isfinite(big).all()
    assert np.array_equal(big[:, 0].cpu().numpy(), np.broadcast_to(c, (B, td)))
    assert float(big.abs().max()) <= 1.0 + 1e-3
    assert max_abs(big[:4].cpu().numpy(), small.cpu().numpy()) <= TOL_LOOP
    assert float((big[1:] - big[:-1]).abs().max()) > 1e-2


@pytest.mark.parametrize("case", LONG_GRAD_CASES, ids=lambda c: c[0])
def test_long_horizon_gradients_vs_reference(case, dev):
    name, net, Hz, T, B, loss_type, pred_eps = case
    g = golden(name)
    od, ad, td, dim, mults = cases.net_dims(net)
    diff = _diffusion(td, od, ad, dim, mults, Hz, T, cases.net_weights(net), dev, loss_type=loss_type,
                      predict_epsilon=pred_eps)
    x0, t, noise = long_train_inputs(name, net, Hz, T, B)
    loss, dx, grads = _backward(diff, x0, t, noise, loss_type, dev)
    loss2, dx2, grads2 = _backward(diff, x0, t, noise, loss_type, dev)
    assert abs(loss - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    wt = {k: torch.from_numpy(v) for k, v in cases.net_weights(net).items()}
    _, og, odx = orc.training_gradients(wt, orc.schedule_buffers("cosine", T), torch.from_numpy(x0), torch.from_numpy(t),
                                        torch.from_numpy(noise), loss_type, pred_eps, None)
    assert set(grads) == set(og)
    worst = 0.0
    for k, got in grads.items():
        assert np.isfinite(got).all(), k
        scale = max(float(g["max." + k]), 1e-12)
        flat = got.reshape(-1)
        idx = cases.grad_sample_index(flat.size)
        e_ref = float(np.max(np.abs(flat[idx].astype(np.float64) - g["g." + k]))) / scale
        e_orc = max_abs(got, og[k].numpy()) / scale
        worst = max(worst, e_ref, e_orc)
        assert e_ref <= REL and e_orc <= REL, f"{k}: rel err vs reference {e_ref:.2e}, vs oracle {e_orc:.2e}"
    sdx = float(np.abs(g["dx"]).max())
    e_dx = max(max_abs(dx, g["dx"]), max_abs(dx, odx.numpy())) / sdx
    print(f"{name}: worst parameter-gradient error {worst:.2e}, d x_t {e_dx:.2e} x max|g|")
    assert e_dx <= REL
    # fixed reduction order across the windowed tiles, the GroupNorm pass and the windowed weight gradients
    assert loss == loss2 and np.array_equal(dx, dx2)
    for k in grads:
        assert np.array_equal(grads[k], grads2[k]), k


@pytest.mark.parametrize("net", [n for n in ORACLE_NETS if n[7] <= 3], ids=lambda n: n[0])
def test_long_horizon_gradients_vs_oracle(net, dev):
    from dynamics_aware_diffusion_amd.utils import synth
    name, od, ad, dim, mults, H, ks, B = net
    td, T = od + ad, 20
    state = synth.synth_unet_state(td, dim, mults, seed=33, kernel_size=ks, affine_jitter=0.25)
    diff = _diffusion(td, od, ad, dim, mults, H, T, state, dev, ks=ks)
    x0 = np.clip(synth.normal_like(26, name + ".x0", (B, H, td)) * 0.5, -1, 1).astype(np.float32)
    t = np.minimum(np.arange(B, dtype=np.int64) * 9, T - 1)
    noise = synth.normal_like(26, name + ".noise", (B, H, td))
    _, dx, grads = _backward(diff, x0, t, noise, "l2", dev)
    _, og, odx = orc.training_gradients(as_torch(state), orc.schedule_buffers("cosine", T), torch.from_numpy(x0),
                                        torch.from_numpy(t), torch.from_numpy(noise), "l2", True, None)
    scales = grad_scales(og)
    worst, worst_key = 0.0, None
    for k, got in grads.items():
        e = max_abs(got, og[k].numpy()) / scales[k]
        if e > worst:
            worst, worst_key = e, k
    e_dx = max_abs(dx, odx.numpy()) / float(odx.abs().max())
    print(f"{name}: worst parameter-gradient error {worst:.2e} x max|g| ({worst_key}), d x_t {e_dx:.2e}")
    assert worst <= REL and e_dx <= REL
