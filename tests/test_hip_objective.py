"""GPU parity of the fused training objective (``GaussianDiffusion.fused_objective = True``): q_sample, the time
MLPs forward and backward, the denoiser and the weighted L1 / L2 mean inside the library
(dad_train_objective_forward / dad_train_objective_backward, csrc/train_objective.hpp) as one autograd node over the
parameters — against the reference's gradient fixtures, the oracle's autograd and the unfused path.

Gates are those of tests/test_hip_train.py and tests/test_hip_train_batch.py: per tensor
|g - g_ref| <= 2e-5 * max|g_ref| (scales from tests/util.grad_scales), loss 2e-6 relative, denoiser output TOL_STEP.
"""
import contextlib

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_hip_parity import TOL_STEP, build, dev, injected_noise  # noqa: F401  (dev: fixture)
from tests.util import as_torch, golden, grad_scales, max_abs, net_weights_torch

pytestmark = pytest.mark.gpu

REL = 2e-5


@contextlib.contextmanager
def fused(diff, on=True):
    """The flag on for the block (the models of ``build`` are shared between tests: it is always put back)."""
    before = diff.fused_objective
    diff.fused_objective = on
    try:
        yield diff
    finally:
        diff.fused_objective = before


def _fresh(net, T, dev, horizon=cases.H, **kw):
    """A GaussianDiffusion of its own (not the shared one of ``build``)."""
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    od, ad, td, dim, mults = cases.net_dims(net)
    unet = TemporalUnet(td, dim=dim, dim_mults=mults, time_dim=cases.net_time_dim(net), kernel_size=cases.net_kernel_size(net))
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in cases.net_weights(net).items()})
    return GaussianDiffusion(unet, horizon, od, ad, n_timesteps=T, **kw).to(dev)


def _step(diff, x0, t, noise, wts, devc, scale=None):
    """diff.loss(x0[, weights]).backward() on injected draws, exactly as _loss_and_backward of test_hip_train.py:
    (loss tensor, {key: gradient})."""
    tt = torch.from_numpy(t).to(devc)
    for p in diff.parameters():
        p.grad = None
    real_randint = torch.randint
    torch.randint = lambda *a, **k: tt.clone()
    try:
        with injected_noise(noise[None], devc), torch.enable_grad():
            loss = diff.loss(torch.from_numpy(x0).to(devc), None if wts is None else torch.from_numpy(wts).to(devc))
            assert loss.requires_grad
            (loss if scale is None else scale * loss).backward()
    finally:
        torch.randint = real_randint
    torch.cuda.synchronize()
    return loss, {k: p.grad.detach().cpu().numpy().copy() for k, p in diff.model.named_parameters()}


def _is_fused(loss):
    return type(loss.grad_fn).__name__ == "_ObjectiveFunctionBackward"


def _assert_close_to_oracle(label, grads, og, rel=REL):
    scales = grad_scales(og)
    assert set(grads) == set(og)
    worst, worst_key = 0.0, None
    for k, got in grads.items():
        assert np.isfinite(got).all(), k
        e = max_abs(got, og[k].numpy()) / scales[k]
        if e > worst:
            worst, worst_key = e, k
    print(f"{label}: worst parameter-gradient error {worst:.2e} x max|g| ({worst_key})")
    bad = {k: f"{max_abs(g, og[k].numpy()) / scales[k]:.2e}" for k, g in grads.items() if not max_abs(g, og[k].numpy()) / scales[k] <= rel}
    assert not bad, f"{label}: farther than {rel} x max|g| from the oracle: {bad}"


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("case", cases.GRAD_CASES, ids=lambda c: c[0])
def test_fused_gradients_vs_reference(case, dev):
    """Every parameter, time MLPs included, against the reference's sampled gradients, its sums and the oracle's
    autograd; the loss against the reference's."""
    from oracle import denoiser as orc
    name, net, T, B, loss_type, pred_eps, weighted = case
    g = golden(name)
    diff = build(net, T, "cosine", dev, loss_type=loss_type, predict_epsilon=pred_eps)
    x0, t, noise, wts = cases.train_inputs(name, net, T, B, weighted)
    with fused(diff):
        loss, grads = _step(diff, x0, t, noise, wts, dev)
    assert _is_fused(loss)
    print(f"{name}: loss {float(loss):.8f} vs reference {float(g['loss']):.8f}")
    assert abs(float(loss) - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    _, og, _ = orc.training_gradients(net_weights_torch(net), orc.schedule_buffers("cosine", T), torch.from_numpy(x0),
                                      torch.from_numpy(t), torch.from_numpy(noise), loss_type, pred_eps,
                                      None if wts is None else torch.from_numpy(wts))
    assert set(grads) == set(og)
    assert any(k.startswith("time_mlp.") for k in grads) and any(".time_mlp.1." in k for k in grads)
    worst, worst_key = 0.0, None
    for k, got in grads.items():
        assert np.isfinite(got).all(), k
        scale = max(float(g["max." + k]), 1e-12)
        flat = got.reshape(-1)
        idx = cases.grad_sample_index(flat.size)
        e_ref = float(np.max(np.abs(flat[idx].astype(np.float64) - g["g." + k]))) / scale
        e_orc = max_abs(got, og[k].numpy()) / scale
        e_sum = abs(float(flat.astype(np.float64).sum()) - float(g["sum." + k])) / (scale * max(1.0, np.sqrt(flat.size)))
        if max(e_ref, e_orc) > worst:
            worst, worst_key = max(e_ref, e_orc), k
        assert e_ref <= REL and e_orc <= REL, f"{k}: rel err vs reference {e_ref:.2e}, vs oracle {e_orc:.2e}"
        assert e_sum <= REL, f"{k}: sum of the gradient off by {e_sum:.2e} (relative to max|g| sqrt(n))"
    print(f"{name}: worst parameter-gradient error {worst:.2e} x max|g| ({worst_key})")


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("case", [
    ("td64", "tiny_td64", cases.H, 5, True),          # time_dim (64) != dim (32)
    ("x0", "tiny", cases.H, 5, False),                # predict_epsilon = False: the target is x_0
    ("H24", "tiny", 24, 3, True),                     # horizon 24, zero-padded to 32
], ids=lambda c: c[0])
def test_fused_gradients_vs_oracle(case, dev):
    from oracle import denoiser as orc
    label, net, H, B, pred_eps = case
    T = 20
    diff = _fresh(net, T, dev, horizon=H, predict_epsilon=pred_eps)
    if label == "x0":
        name = "train_tiny_x0_l2"
        x0, t, noise, _ = cases.train_inputs(name, net, T, B, False)
    else:
        x0, t, noise, _ = cases.train_inputs("objective." + label, net, T, B, False)
        x0, noise = np.ascontiguousarray(x0[:, :H]), np.ascontiguousarray(noise[:, :H])
    with fused(diff):
        loss, grads = _step(diff, x0, t, noise, None, dev)
    assert _is_fused(loss)
    ol, og, _ = orc.training_gradients(net_weights_torch(net), orc.schedule_buffers("cosine", T), torch.from_numpy(x0),
                                       torch.from_numpy(t), torch.from_numpy(noise), "l2", pred_eps)
    print(f"{label}: loss {float(loss):.8f} vs oracle {float(ol):.8f}")
    assert abs(float(loss) - float(ol)) <= 2e-6 * max(1.0, abs(float(ol)))
    if label == "x0":
        want = float(golden("training")["train_tiny_x0_l2.loss"])
        assert abs(float(loss) - want) <= 2e-6 * max(1.0, abs(want))
    _assert_close_to_oracle(label, grads, og)


# ------------------------------------------------------------------------------------------------ 3
def test_fused_pointmaze_batch_250_vs_float64(dev):
    """The PointMaze net at B = 250 (ragged against every tile of the time chain: 250 = 7 * 32 + 26), against the
    oracle in float64; criterion of test_large_batch_gradients_vs_float64."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    from tests.test_hip_long_horizon import _diffusion
    td, dim, mults, H, B, T = 6, 128, (1, 2, 4), 32, 250, 20
    state = synth.synth_unet_state(td, dim, mults, seed=41, affine_jitter=0.3)
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, state, dev)
    x0 = np.clip(synth.normal_like(20, "objective.x.B250", (B, H, td)) * 0.5, -1, 1).astype(np.float32)
    t = np.array([(3 * i + 1) % T for i in range(B)], dtype=np.int64)
    t[0], t[-1] = 0, T - 1
    noise = synth.normal_like(20, "objective.n.B250", (B, H, td))
    with fused(diff):
        loss, grads = _step(diff, x0, t, noise, None, dev)
    assert _is_fused(loss)
    w64 = orc.cast_weights(as_torch(state), torch.float64)
    s64 = {k: v.double() for k, v in orc.schedule_buffers("cosine", T).items()}
    l64, g64, _ = orc.training_gradients(w64, s64, torch.from_numpy(x0).double(), torch.from_numpy(t), torch.from_numpy(noise).double())
    e_loss = abs(float(loss) - float(l64)) / max(1.0, abs(float(l64)))
    print(f"B250: loss {float(loss):.8f}, {e_loss:.1e} relative from float64")
    assert e_loss <= 2e-6
    _assert_close_to_oracle("pointmaze B=250 vs float64", grads, g64)


# ------------------------------------------------------------------------------------------------ 4
def test_x_t_equals_q_sample_bit_for_bit(dev):
    """The x_t the library formed (read back from the saved region) equals diffusion.q_sample(x0, t, noise) bit for
    bit; the denoiser output it kept agrees with diffusion.model(q_sample(...), t) within TOL_STEP; under no_grad the
    fused forward alone is the validation loss."""
    name, net, T, B = "grads_tiny", "tiny", 20, 6
    diff = build(net, T, "cosine", dev, loss_type="l2", predict_epsilon=True)
    x0, t, noise, _ = cases.train_inputs(name, net, T, B, False)
    x0t, tt, nz = torch.from_numpy(x0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(noise).to(dev)
    diff._engine(dev)                      # (binds the schedule and the diffusion's options to the model)
    eng = diff.model.engine(cases.H, dev, training=True)
    eng.bind_train_schedule(diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod)
    loss, saved = eng.objective_forward(x0t, tt.to(torch.int32), nz, None, 2)
    xt, out = eng.objective_saved_views(saved, B)
    with torch.no_grad():
        want_xt = diff.q_sample(x0t, tt, nz)
        want_out = diff.model(want_xt, tt)
        want_loss = ((want_out - nz) ** 2).mean()
    torch.cuda.synchronize()
    assert torch.equal(xt, want_xt), f"x_t differs from q_sample by {float((xt - want_xt).abs().max()):.3e}"
    e_out = float((out - want_out).abs().max())
    print(f"denoiser output of the fused forward vs model(q_sample): {e_out:.2e}")
    assert e_out <= TOL_STEP
    assert abs(float(loss) - float(want_loss)) <= 2e-6 * max(1.0, abs(float(want_loss)))
    # timesteps outside the schedule are clamped before any table read
    wild = tt.to(torch.int32).clone()
    wild[0], wild[1] = -7, T + 100
    _, saved2 = eng.objective_forward(x0t, wild, nz, None, 2)
    clamped = tt.clone()
    clamped[0], clamped[1] = 0, T - 1
    torch.cuda.synchronize()
    assert torch.equal(eng.objective_saved_views(saved2, B)[0], diff.q_sample(x0t, clamped, nz))
    # validation loss: no graph
    real_randint = torch.randint
    torch.randint = lambda *a, **k: tt.clone()
    try:
        with fused(diff), injected_noise(noise[None], dev), torch.no_grad():
            val = diff.loss(x0t)
    finally:
        torch.randint = real_randint
    assert not val.requires_grad and float(val) == float(loss)


# ------------------------------------------------------------------------------------------------ 5
def test_structure_one_node_over_the_parameters(dev):
    name, net, T, B, loss_type, pred_eps, weighted = cases.GRAD_CASES[0]
    diff = build(net, T, "cosine", dev, loss_type=loss_type, predict_epsilon=pred_eps)
    x0, t, noise, wts = cases.train_inputs(name, net, T, B, weighted)
    with fused(diff):
        loss, g1 = _step(diff, x0, t, noise, wts, dev)
        assert _is_fused(loss)
        nexts = [fn for fn, _ in loss.grad_fn.next_functions if fn is not None]
        assert len(nexts) == len(list(diff.model.parameters()))
        assert all(type(fn).__name__ == "AccumulateGrad" for fn in nexts), {type(fn).__name__ for fn in nexts}
        assert {id(fn.variable) for fn in nexts} == {id(p) for p in diff.model.parameters()}
        loss2, g2 = _step(diff, x0, t, noise, wts, dev)
    assert float(loss) == float(loss2)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), f"{k} differs between two fresh forward / backward passes"
    # a trajectory that requires grad takes the unfused path; so does a loss_fn the library does not know
    with fused(diff), torch.enable_grad():
        x = torch.from_numpy(x0).to(dev).requires_grad_(True)
        assert not _is_fused(diff.loss(x))
        kept = diff.loss_fn
        diff.loss_fn = torch.nn.SmoothL1Loss(reduction="none")
        try:
            assert not _is_fused(diff.loss(torch.from_numpy(x0).to(dev)))
        finally:
            diff.loss_fn = kept


def test_wrong_tensor_count_is_refused(dev):
    import ctypes as C
    from dynamics_aware_diffusion_amd._engine import DadError
    diff = build("tiny", 20, "cosine", dev, loss_type="l2", predict_epsilon=True)
    diff._engine(dev)                      # (binds the schedule and the diffusion's options to the model)
    eng = diff.model.engine(cases.H, dev, training=True)
    eng.bind_train_schedule(diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod)
    x = torch.zeros(2, cases.H, 6, device=dev)
    loss, saved = eng.objective_forward(x, torch.zeros(2, dtype=torch.int32, device=dev), x, None, 2)
    one = (C.c_void_p * 1)(x.data_ptr())
    for n, nt in ((1, len(eng.time_grad_layout()[0])), (len(eng.grad_layout()[0]), 1)):
        rc = eng.lib.dad_train_objective_backward(eng._h, x.data_ptr(), x.data_ptr(), None, 2, loss.data_ptr(), one, n, one, nt, 2,
                                                  saved.data_ptr(), saved.numel() * 4, saved.data_ptr(), saved.numel() * 4, None)
        assert rc == -1 and b"gradient tensors passed" in eng.lib.dad_last_error()
    with pytest.raises(DadError, match="loss_type"):
        eng.objective_forward(x, torch.zeros(2, dtype=torch.int32, device=dev), x, None, 7)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6
def test_flag_off_is_unchanged_and_on_agrees(dev):
    name, net, T, B = "grads_tiny", "tiny", 20, 6
    diff = _fresh(net, T, dev)
    assert diff.fused_objective is False
    x0, t, noise, _ = cases.train_inputs(name, net, T, B, False)
    l_before, g_before = _step(diff, x0, t, noise, None, dev)       # before the attribute is ever touched
    assert not _is_fused(l_before)
    diff.fused_objective = True
    l_on, g_on = _step(diff, x0, t, noise, None, dev)
    assert _is_fused(l_on)
    diff.fused_objective = False
    l_off, g_off = _step(diff, x0, t, noise, None, dev)
    assert not _is_fused(l_off)
    assert float(l_off) == float(l_before)
    for k in g_before:
        assert np.array_equal(g_before[k], g_off[k]), f"{k}: the default path changed"
    assert abs(float(l_on) - float(l_off)) <= 2e-6 * max(1.0, abs(float(l_off)))
    for k in g_off:
        scale = max(float(np.abs(g_off[k]).max()), 1e-12)
        e = max_abs(g_on[k], g_off[k]) / scale
        assert e <= REL, f"{k}: fused and unfused gradients differ by {e:.2e} x max|g|"


# ------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("net", ["tiny4", "tiny_d48"])
def test_fused_sgd_steps_track_the_oracle(net, dev):
    """Three optimiser steps with the flag on against the oracle's three steps (as
    test_sgd_steps_track_the_oracle_without_leaving_the_device): the fused path reads the refreshed device copies of
    every tensor, time MLPs included, without an engine rebuild."""
    from oracle import denoiser as orc
    T, B, lr = 20, 5, 0.05
    diff = _fresh(net, T, dev)
    diff.fused_objective = True
    opt = torch.optim.SGD(diff.model.parameters(), lr=lr)
    w = {k: v.clone() for k, v in net_weights_torch(net).items()}
    sched = orc.schedule_buffers("cosine", T)
    engines = set()
    for step in range(3):
        x0, t, noise, _ = cases.train_inputs(f"sgd.{step}", net, T, B, False)
        tt = torch.from_numpy(t).to(dev)
        real_randint = torch.randint
        torch.randint = lambda *a, **k: tt.clone()
        try:
            with injected_noise(noise[None], dev), torch.enable_grad():
                opt.zero_grad()
                loss = diff.loss(torch.from_numpy(x0).to(dev))
                assert _is_fused(loss)
                loss.backward()
                opt.step()
        finally:
            torch.randint = real_randint
        engines.add(id(diff.model._engine))
        ol, og, _ = orc.training_gradients(w, sched, torch.from_numpy(x0), torch.from_numpy(t), torch.from_numpy(noise))
        w = {k: v - lr * og[k] for k, v in w.items()}
        assert abs(float(loss) - float(ol)) <= 5e-6 * max(1.0, abs(float(ol))), (step, float(loss), float(ol))
    torch.cuda.synchronize()
    assert len(engines) == 1, "the engine was rebuilt instead of refreshed"
    for k, p in diff.model.named_parameters():
        assert max_abs(p.detach().cpu().numpy(), w[k].numpy()) <= 2e-5 * max(1.0, float(w[k].abs().max())), k


def test_refreshed_time_mlp_copies_are_read(dev):
    """The same draws before and after an optimiser step give different losses, and the second is the oracle's on the
    stepped weights: the fused forward reads the re-derived device copies of the time-MLP tensors."""
    from oracle import denoiser as orc
    net, T, B, lr = "tiny", 20, 5, 0.5
    diff = _fresh(net, T, dev)
    diff.fused_objective = True
    time_params = [p for k, p in diff.model.named_parameters() if "time_mlp." in k]
    opt = torch.optim.SGD(time_params, lr=lr)          # only the time MLPs move
    x0, t, noise, _ = cases.train_inputs("objective.refresh", net, T, B, False)
    opt.zero_grad()
    l1, g1 = _step(diff, x0, t, noise, None, dev)
    opt.step()
    l2, _ = _step(diff, x0, t, noise, None, dev)
    w = {k: v.clone() for k, v in net_weights_torch(net).items()}
    for k in w:
        if "time_mlp." in k:
            w[k] = w[k] - lr * torch.from_numpy(g1[k])
    ol, _, _ = orc.training_gradients(w, orc.schedule_buffers("cosine", T), torch.from_numpy(x0), torch.from_numpy(t),
                                      torch.from_numpy(noise))
    print(f"loss before / after a time-MLP step: {float(l1):.8f} / {float(l2):.8f} (oracle {float(ol):.8f})")
    assert float(l2) != float(l1)
    assert abs(float(l2) - float(ol)) <= 5e-6 * max(1.0, abs(float(ol)))


def test_composed_loss_with_the_flag_on(dev):
    """ComposedLoss([DiffusionLoss, ProjectionLoss]).backward() with the flag on gives the diffusion term's gradients
    (as test_composed_loss_backward)."""
    import io
    from dynamics_aware_diffusion_amd.dynamics import ProjectionMatrixBuilder, double_integrator
    from dynamics_aware_diffusion_amd.losses import ComposedLoss, DiffusionLoss, ProjectionLoss
    name, net, T, B, loss_type, pred_eps, weighted = cases.GRAD_CASES[0]
    g = golden(name)
    diff = build(net, T, "cosine", dev, loss_type=loss_type, predict_epsilon=pred_eps)
    A, Bm = double_integrator(0.1)
    with contextlib.redirect_stdout(io.StringIO()):
        P = ProjectionMatrixBuilder(A, Bm, 4, 2).get_projection_matrix(cases.H)
        terms = ComposedLoss([DiffusionLoss(diff, 1.0),
                              ProjectionLoss(P, cases.NormalizerStub(4, 2), state_dim=4, action_dim=2, observation_dim=4,
                                             horizon=cases.H, weight=0.1, device=str(dev))])
    x0, t, noise, _ = cases.train_inputs(name, net, T, B, weighted)
    tt = torch.from_numpy(t).to(dev)
    for p in diff.parameters():
        p.grad = None
    real_randint = torch.randint
    torch.randint = lambda *a, **k: tt.clone()
    try:
        with fused(diff), injected_noise(noise[None], dev), torch.enable_grad():
            total, parts = terms({"conditions": torch.from_numpy(x0).to(dev)})
            total.backward()
    finally:
        torch.randint = real_randint
    torch.cuda.synchronize()
    assert abs(parts["diffusion"] - float(g["loss"])) <= 2e-6 * max(1.0, abs(float(g["loss"])))
    for k, p in diff.model.named_parameters():
        flat = p.grad.cpu().numpy().reshape(-1)
        idx = cases.grad_sample_index(flat.size)
        assert float(np.max(np.abs(flat[idx] - g["g." + k]))) <= REL * max(float(g["max." + k]), 1e-12), k


# ------------------------------------------------------------------------------------------------ 8
def test_scaled_incoming_gradient(dev):
    """(0.37 * diff.loss(x)).backward() gives 0.37 x the gradients of the plain step: autograd's incoming scalar is
    read on the device."""
    name, net, T, B, loss_type, pred_eps, weighted = cases.GRAD_CASES[0]
    diff = build(net, T, "cosine", dev, loss_type=loss_type, predict_epsilon=pred_eps)
    x0, t, noise, wts = cases.train_inputs(name, net, T, B, weighted)
    with fused(diff):
        _, g1 = _step(diff, x0, t, noise, wts, dev)
        _, gs = _step(diff, x0, t, noise, wts, dev, scale=0.37)
    for k in g1:
        scale = max(float(np.abs(g1[k]).max()), 1e-12)
        e = max_abs(gs[k], np.float32(0.37) * g1[k]) / (0.37 * scale)
        assert e <= REL, f"{k}: {e:.2e} x max|g| from 0.37 x the unscaled gradient"
        assert float(np.abs(gs[k]).max()) < 0.5 * scale + 1e-30, k
