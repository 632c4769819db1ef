"""``losses.DynamicsAwareLoss`` on the device: the diffusion term and the dynamics violation of the predicted plan from
one evaluation of the denoiser, on both routes (default: the existing autograd nodes; library:
dad_train_dynamics_objective_forward / _backward as one node).

(a) float64 truth, both routes: every parameter gradient (time MLPs included), the two parts and the total against
    float64 autograd through ``oracle.denoiser.unet_forward`` and the restated violation.  Gates are the project's own:
    per tensor ``|g - g64| <= REL * max|g64|`` with REL = 2e-5 (tests/test_hip_train.py), the diffusion part 5e-6 and the
    projection part 2e-5 relative (tests/test_hip_violation_grad.py::test_training_with_predicted_projection_loss, which
    measures 1.7e-6 for the parent's two-pass form on the same net).
(b) the default route makes ``GaussianDiffusion.loss``'s draws: with one weight zero it is bit-equal to the other
    term's existing form under the same seed, and it consumes the device generator as one ``diffusion.loss`` call does.
(c) two library-route runs give the same bits; a second backward with ``retain_graph=True`` behaves as
    ``_ObjectiveFunction``'s does.
(d) ``Trainer`` with ``FusedAdam`` takes three steps through the new loss.

A timestep outside the schedule is clamped by the library (as ``objective_xt_kernel`` clamps it); torch's gather on the
default route would fault on it, so in the clamping case the default route is handed the clamped vector and only the
library route the raw one.
"""
import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_hip_objective import _fresh
from tests.test_hip_parity import dev, injected_noise  # noqa: F401  (dev: fixture)
from tests.test_hip_train import REL
from tests.test_hip_violation_grad import _violation
from tests.util import net_weights_torch

pytestmark = pytest.mark.gpu

T = 20
PW = 0.1


def _projection(net, H, seed=9):
    """The non-symmetric random projector and statistics of test_hip_violation_grad._tiny_projection, for any net."""
    od, ad, td, dim, mults = cases.net_dims(net)
    g = torch.Generator().manual_seed(seed)
    D = (H + 1) * od + H * ad
    P = torch.randn(D, D, generator=g) / D ** 0.5
    stats = (torch.randn(od, generator=g), 0.5 + torch.rand(od, generator=g),
             torch.randn(ad, generator=g), 0.5 + torch.rand(ad, generator=g))
    norm = cases.NormalizerStub(od, ad)
    norm.obs_mean, norm.obs_std, norm.action_mean, norm.action_std = (s.numpy() for s in stats)
    return od, ad, D, P, stats, norm


def _loss(diff, net, H, devc, pw=PW, dw=1.0, tw=None, seed=9):
    from dynamics_aware_diffusion_amd.losses import DynamicsAwareLoss
    od, ad, D, P, stats, norm = _projection(net, H, seed)
    loss = DynamicsAwareLoss(diff, P, norm, state_dim=od, action_dim=ad, observation_dim=od, horizon=H,
                             projection_weight=pw, diffusion_weight=dw, timestep_weights=tw, device=str(devc))
    return loss, (od, ad, D, P, stats)


def _run(loss, x0, t, noise, wts, devc, scale=None, retain=False):
    """loss(batch)[0].backward() on injected draws: (total, parts, {key: gradient})."""
    diff = loss.diffusion
    tt = torch.from_numpy(t).to(devc)
    for p in diff.parameters():
        p.grad = None
    batch = {"conditions": torch.from_numpy(x0).to(devc)}
    if wts is not None:
        batch["weights"] = torch.from_numpy(wts).to(devc)
    real_randint = torch.randint
    torch.randint = lambda *a, **k: tt.clone()
    try:
        with injected_noise(noise[None], devc), torch.enable_grad():
            total, parts = loss(batch)
            assert total.requires_grad and list(parts) == ["diffusion", "projection", "total"]
            (total if scale is None else scale * total).backward(retain_graph=retain)
    finally:
        torch.randint = real_randint
    torch.cuda.synchronize()
    return total, parts, {k: p.grad.detach().cpu().double() for k, p in diff.model.named_parameters()}


def _truth(net, proj, x0, t, noise, wts, tw, pred_eps, loss_type, pw, dw, scale):
    """float64 autograd through the oracle: (Ld, pw * Lp, total, {key: gradient of scale * total})."""
    from oracle import denoiser as orc
    od, ad, D, P, stats = proj
    B = x0.shape[0]
    w64 = {k: v.double().requires_grad_(True) for k, v in net_weights_torch(net).items()}
    sched = {k: v.double() for k, v in orc.schedule_buffers("cosine", T).items()}
    x64, n64, t64 = torch.from_numpy(x0).double(), torch.from_numpy(noise).double(), torch.from_numpy(t)
    at = lambda key: sched[key].gather(-1, t64).reshape(B, 1, 1)          # noqa: E731
    with torch.enable_grad():
        xt = at("sqrt_alphas_cumprod") * x64 + at("sqrt_one_minus_alphas_cumprod") * n64
        out = orc.unet_forward(w64, xt, t64)
        d = out - (n64 if pred_eps else x64)
        el = d.abs() if loss_type == "l1" else d ** 2
        if wts is not None:
            el = el * torch.from_numpy(wts).double()
        ld = el.mean()
        x0_hat = at("sqrt_recip_alphas_cumprod") * xt - at("sqrt_recipm1_alphas_cumprod") * out if pred_eps else out
        viol = _violation(x0_hat, P, od, od, stats)
        if tw is not None:
            viol = viol * tw.double()[t64]
        lp = pw * (viol.sum() / (B * D))
        total = dw * ld + lp
        (scale * total).backward()
    return float(ld), float(lp), float(total), {k: v.grad for k, v in w64.items()}


#        id           net        H   B   form    eps    loss  wts    tw     wild   g
CASES = [
    ("base",         "tiny",     32, 4,  None,   True,  "l2", False, False, False, 1.0),
    ("gemm_B33",     "tiny",     32, 33, "gemm", True,  "l2", False, False, False, 1.0),   # second row tile holds one trajectory; D = 196 = 6 * 32 + 4
    ("x0",           "tiny",     32, 4,  None,   False, "l2", False, False, False, 1.0),
    ("l1_w_tw_t_g3", "tiny",     32, 5,  None,   True,  "l1", True,  True,  True,  3.0),   # weights, timestep weights, t = 0 / T-1 / outside, g = 3
    ("x0_gemm_l1",   "tiny",     32, 5,  "gemm", False, "l1", True,  True,  False, 3.0),
    ("H24",          "tiny",     24, 3,  None,   True,  "l2", False, False, False, 1.0),   # zero-padded horizon
    ("d24",          "tiny_d24", 32, 4,  None,   True,  "l2", False, True,  False, 1.0),   # zero-padded GroupNorm groups
    ("d24_gemm",     "tiny_d24", 32, 4,  "gemm", True,  "l2", False, False, False, 1.0),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_both_routes_vs_float64(case, dev):
    name, net, H, B, form, pred_eps, loss_type, weighted, use_tw, wild, g = case
    diff = _fresh(net, T, dev, horizon=H, predict_epsilon=pred_eps, loss_type=loss_type)
    x0, t, noise, wts = cases.train_inputs("dynobj." + name, net, T, B, weighted)
    x0, noise = np.ascontiguousarray(x0[:, :H]), np.ascontiguousarray(noise[:, :H])
    if wts is not None:
        wts = np.ascontiguousarray(wts[:, :H])
    tw = None
    if use_tw:
        tw = torch.linspace(1.0, 0.05, T) ** 2
        tw[3] = 0.0
    t_raw = t.copy()
    if wild:
        t_raw[0], t_raw[1], t_raw[2], t_raw[3] = 0, T - 1, T + 100, -7
    t_clamped = np.clip(t_raw, 0, T - 1)
    loss, proj = _loss(diff, net, H, dev, tw=tw)
    loss.form = form
    want_form = form or "row"
    ld, lp, tot, g64 = _truth(net, proj, x0, t_clamped, noise, wts, tw, pred_eps, loss_type, PW, 1.0, g)
    for route in ("default", "library"):
        diff.fused_objective = route == "library"
        assert loss.route(B)[0] == route, loss.route(B)
        total, parts, grads = _run(loss, x0, t_raw if route == "library" else t_clamped, noise, wts, dev, scale=g)
        assert loss.last_route == route
        plan = diff.model.engine(H, dev, training=True).dynamics_objective_plan(B, state=loss._state, form=form)
        assert plan["form"] == want_form and not plan["refused"] and plan["D"] == proj[2] and plan["horizon"] == H
        assert plan["launches"][0]["kind"] == "fwd_" + want_form and plan["launches"][2]["kind"] == "bwd_" + want_form
        if route == "library":
            assert type(total.grad_fn).__name__ == "SelectBackward0"
            assert type(total.grad_fn.next_functions[0][0]).__name__ == "_DynamicsObjectiveFunctionBackward"
        e_d = abs(parts["diffusion"] - ld) / max(1.0, abs(ld))
        e_p = abs(parts["projection"] - lp) / max(1.0, abs(lp))
        e_t = abs(parts["total"] - tot) / max(1.0, abs(tot))
        assert set(grads) == set(g64)
        errs = {k: float((grads[k] - g64[k]).abs().max() / max(float(g64[k].abs().max()), 1e-12)) for k in grads}
        worst = max(errs, key=errs.get)
        print(f"\n{name} [{route}, {want_form}]: diffusion {parts['diffusion']:.6f} ({e_d:.1e}), projection {parts['projection']:.6f} "
              f"({e_p:.1e}), total ({e_t:.1e}); worst gradient {errs[worst]:.2e} x max|g| ({worst})")
        assert float(total) == parts["total"]
        assert e_d <= 5e-6 and e_p <= 2e-5 and e_t <= 2e-5
        assert all(torch.isfinite(v).all() for v in grads.values())
        bad = {k: f"{e:.2e}" for k, e in errs.items() if not e <= REL}
        assert not bad, f"{name} [{route}]: farther than {REL} x max|g| from float64: {bad}"


def _seeded(fn, devc, seed=4321):
    torch.manual_seed(seed)
    out = fn()
    return out, torch.randn(4, device=devc)


def test_default_route_makes_the_draws_of_diffusion_loss(dev):
    from dynamics_aware_diffusion_amd.losses import PredictedProjectionLoss
    net, H, B = "tiny", cases.H, 4
    diff = _fresh(net, T, dev)
    x0, _, _, _ = cases.train_inputs("dynobj.draws", net, T, B, False)
    x = torch.from_numpy(x0).to(dev)
    params = dict(diff.model.named_parameters())

    def grads_of(make):
        for p in diff.parameters():
            p.grad = None
        with torch.enable_grad():
            value = make()
            value.backward()
        return value.detach(), {k: p.grad.clone() for k, p in params.items()}

    # projection_weight = 0: the diffusion term alone
    only_d, _ = _loss(diff, net, H, dev, pw=0.0)
    (want, want_g), next_a = _seeded(lambda: grads_of(lambda: diff.loss(x)), dev)
    parts = {}
    (got, got_g), next_b = _seeded(lambda: grads_of(lambda: parts.setdefault("o", only_d({"conditions": x}))[0]), dev)
    assert only_d.last_route == "default"
    assert torch.equal(next_a, next_b), "the call does not consume the generator as one diffusion.loss call does"
    assert parts["o"][1]["diffusion"] == float(want) and torch.equal(got, want)
    assert all(torch.equal(got_g[k], want_g[k]) for k in params)
    # diffusion_weight = 0: the projection term alone
    od, ad, D, P, stats, norm = _projection(net, H)
    ppl = PredictedProjectionLoss(diff, P, norm, state_dim=od, action_dim=ad, observation_dim=od, horizon=H, weight=PW, device=str(dev))
    only_p, _ = _loss(diff, net, H, dev, pw=PW, dw=0.0)
    (want, want_g), next_c = _seeded(lambda: grads_of(lambda: ppl({"conditions": x})), dev)
    parts = {}
    (got, got_g), next_d = _seeded(lambda: grads_of(lambda: parts.setdefault("o", only_p({"conditions": x}))[0]), dev)
    assert torch.equal(next_c, next_d) and torch.equal(next_a, next_c)
    assert parts["o"][1]["projection"] == float(want) and torch.equal(got, want)
    assert all(torch.equal(got_g[k], want_g[k]) for k in params)


def test_library_route_is_deterministic_and_its_graph_is_spent_once(dev):
    net, H, B = "tiny", cases.H, 5
    diff = _fresh(net, T, dev)
    diff.fused_objective = True
    x0, t, noise, _ = cases.train_inputs("dynobj.twice", net, T, B, False)
    runs = []
    for form in (None, "gemm"):
        loss, _ = _loss(diff, net, H, dev, tw=torch.linspace(1.0, 0.1, T))
        loss.form = form
        a = _run(loss, x0, t, noise, None, dev)
        b = _run(loss, x0, t, noise, None, dev)
        assert loss.last_route == "library" and a[1] == b[1]
        assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])
        runs.append(a)
    # the two forms add in different orders: close, not equal
    assert abs(runs[0][1]["projection"] - runs[1][1]["projection"]) <= 2e-5 * max(1.0, abs(runs[0][1]["projection"]))
    # a second backward through a retained graph: what _ObjectiveFunction's does (its saved state is dropped by the first)
    xs = torch.from_numpy(x0).to(dev)

    def second_backward(make):
        with torch.enable_grad():
            value = make()
            value.backward(retain_graph=True)
            try:
                value.backward()
            except Exception as e:                 # noqa: BLE001
                return type(e)
        return None

    loss, _ = _loss(diff, net, H, dev)
    assert second_backward(lambda: loss({"conditions": xs})[0]) is second_backward(lambda: diff.loss(xs))


def test_trainer_takes_steps_through_the_new_loss(dev, tmp_path):
    from dynamics_aware_diffusion_amd.utils import synth
    from dynamics_aware_diffusion_amd.utils.training import FusedAdam, Trainer
    from tests.test_hip_optim import _plan, _tiny
    for fused_objective in (False, True):
        diff = _tiny(dev)
        diff.fused_objective = fused_objective
        od, ad = synth.ARCHS["tiny"][:2]
        td, Tn = od + ad, int(diff.n_timesteps)
        g = torch.Generator().manual_seed(3)
        D = 33 * od + 32 * ad
        norm = cases.NormalizerStub(od, ad)
        tw = (torch.arange(Tn) < Tn // 2).float()
        from dynamics_aware_diffusion_amd.losses import DynamicsAwareLoss
        loss = DynamicsAwareLoss(diff, torch.randn(D, D, generator=g) / D ** 0.5, norm, state_dim=od, action_dim=ad,
                                 observation_dim=od, horizon=32, projection_weight=0.05, timestep_weights=tw, device=str(dev))
        tr = Trainer(diff, FusedAdam(list(diff.parameters()), lr=1e-3), None, device=dev, log_dir=str(tmp_path / str(fused_objective)),
                     use_ema=True, ema_decay=0.5, gradient_clip=1.0, loss_fn=loss, loss_names=["diffusion", "projection", "total"])
        noise = torch.from_numpy(synth.normal_like(9, "dynobj.plan.noise", (Tn + 1, 2, 32, td)))
        before_plan = _plan(tr.ema_model, noise, dev)
        p0 = [p.detach().clone() for p in diff.model.parameters()]
        e0 = [p.detach().clone() for p in tr.ema_model.parameters()]
        for k in range(3):
            x0 = torch.from_numpy(synth.normal_like(9, f"dynobj.batch.{k}", (4, 32, td)))
            torch.manual_seed(50 + k)
            parts = tr.train_step({"conditions": x0})
            assert list(parts) == ["diffusion", "projection", "total"] and all(np.isfinite(v) for v in parts.values())
            assert loss.last_route == ("library" if fused_objective else "default")
        assert any(not torch.equal(a, b) for a, b in zip(p0, diff.model.parameters()))
        assert any(not torch.equal(a, b) for a, b in zip(e0, tr.ema_model.parameters()))
        after_plan = _plan(tr.ema_model, noise, dev)
        assert np.isfinite(after_plan).all() and not np.array_equal(before_plan, after_plan)
        tr.log_file.close()

