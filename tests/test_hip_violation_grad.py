"""GPU tests of the differentiable dynamics violation (``dad_projection_violation_fwd`` / ``_bwd``,
``ProjectionState.violation_fn``, ``losses.ProjectionLoss`` under autograd, ``losses.PredictedProjectionLoss``, the
violation as a guide).

Oracle: float64 torch autograd of the reference's expression (ProjectionLoss.compute,
m_diffuser/losses/__init__.py:161-186: gather, cat, ``@ P``, square, sum), restated in ``_violation``.  The projector is
random and NOT symmetric (entries ~ N(0, 1/D)): a kernel that multiplied by P where P^T belongs fails by O(1).

Criterion for the value (a) and the gradient (b): the same expression and its autograd are evaluated in fp32 on the CPU
too; with e_ref its worst error against float64 and e_hip the kernels', both in units of max |viol| resp. max |g|,

    e_hip <= max(4 e_ref, 8 * 2^-24)

— 4: a different but equally long summation order (four waves over 64-wide chunks against torch's blocking, plus the
fixed-order partial sums); the floor: the handful of roundings of the 2 w std scaling and the two-term sum of the last
state, for a D so small that e_ref happens to vanish.

Measured on an MI355X (e_hip / e_ref; value, then gradient):
    row_D52_B3            5.08e-08 / 6.42e-08    6.08e-08 / 1.39e-07
    row_D196_B5           3.76e-08 / 3.76e-08    7.34e-08 / 1.88e-07
    row_od6               1.13e-07 / 8.71e-08    9.90e-08 / 1.36e-07
    gemm_D52_B32          5.67e-08 / 8.07e-08    9.83e-08 / 1.11e-07
    gemm_D514_B33         1.64e-07 / 1.18e-07    1.90e-07 / 2.66e-07
    gemm_D2410_B32        1.79e-07 / 1.25e-07    3.15e-07 / 1.80e-07
    gemm_D2410_B2         2.21e-07 / 3.93e-08    4.21e-07 / 6.51e-07
    row_vs_gemm_D196_B64  row 7.64e-08, gemm 9.66e-08 / 1.24e-07;  row 1.09e-07, gemm 1.81e-07 / 2.28e-07;
                          |row - gemm| 1.73e-07 (value), 2.54e-07 (gradient)
    ProjectionLoss.backward  gradient 1.08e-07 / 1.28e-07
    PredictedProjectionLoss  worst parameter gradient 1.66e-06 (eps), 1.74e-06 (x0) x max |g|, against REL = 2e-5
    guided step              |policy - engine(g64)| 1.19e-07 against a tolerance of 4.84e-07
"""
import functools

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_hip_parity import build, dev, injected_noise  # noqa: F401  (dev: fixture)
from tests.test_hip_train import REL
from tests.util import net_weights_torch

pytestmark = pytest.mark.gpu

FLOOR = 8 * 2.0 ** -24
SENTINEL = 12345.0


def _bound(e_ref):
    return max(4.0 * e_ref, FLOOR)


def _violation(x, P, n, od, stats):
    """ProjectionLoss.compute (losses/__init__.py:161-186) before its mean, per row, in x's dtype: the first n observation
    channels are the state (the reference has od == n)."""
    om, osd, am, asd = (s.to(x.dtype) for s in stats)
    s = x[:, :, :n] * osd[:n] + om[:n]
    a = x[:, :, od:] * asd + am
    v = torch.cat([torch.cat([s, s[:, -1:]], dim=1).reshape(x.shape[0], -1), a.reshape(x.shape[0], -1)], dim=1)
    return ((v - v @ P.to(x.dtype)) ** 2).sum(dim=1)


def _value_and_grad(x, w, P, n, od, stats, dtype):
    with torch.enable_grad():                  # (the suite runs under no_grad)
        xx = x.detach().clone().to(dtype).requires_grad_(True)      # (a copy: .to() of the same dtype is x itself)
        viol = _violation(xx, P, n, od, stats)
        (viol * w.to(dtype)).sum().backward()
    return viol.detach(), xx.grad.detach()


@functools.lru_cache(None)
def _inputs(n, od, m, H, B, seed):
    """(x, w, P, stats) on the host, fp32, and the float64 / fp32 CPU results: computed once per shape, never changed."""
    g = torch.Generator().manual_seed(seed)
    D = (H + 1) * n + H * m
    P = torch.randn(D, D, generator=g) / D ** 0.5
    x = torch.randn(B, H, od + m, generator=g)
    stats = (torch.randn(od, generator=g), 0.5 + torch.rand(od, generator=g),
             torch.randn(m, generator=g), 0.5 + torch.rand(m, generator=g))
    w = torch.randn(B, generator=g)
    w[0] = abs(w[0]) + 0.5                     # positive, negative and exactly-zero rows
    if B > 1:
        w[1] = -abs(w[1]) - 0.5
    if B > 2:
        w[2] = 0.0
    v64, g64 = _value_and_grad(x, w, P, n, od, stats, torch.float64)
    v32, g32 = _value_and_grad(x, w, P, n, od, stats, torch.float32)
    e_ref_v = float((v32.double() - v64).abs().max() / v64.abs().max())
    e_ref_g = float((g32.double() - g64).abs().max() / g64.abs().max())
    return x, w, P, stats, v64, g64, e_ref_v, e_ref_g


def _state(P, stats, n, od, m, dev):
    from dynamics_aware_diffusion_amd._engine import ProjectionState
    return ProjectionState(P, stats[0], stats[1], stats[2], stats[3], n, od, m, dev)


def _round64(floats):
    return (floats + 63) // 64 * 64


def _run(st, x_dev, w_dev, form):
    """One forward + backward through violation_fn on a workspace full of SENTINEL; (viol, d_x, workspace)."""
    B, H = x_dev.shape[0], x_dev.shape[1]
    need = st.grad_plan(B, H, "gemm")["workspace_bytes"] // 4             # (the larger of the two forms')
    st._vg_ws = torch.full((need,), SENTINEL, dtype=torch.float32, device=x_dev.device)
    with torch.enable_grad():
        x = x_dev.clone().requires_grad_(True)
        viol = st.violation_fn(x, form)
        assert viol.requires_grad and viol.shape == (B,)
        (viol * w_dev).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(x.detach(), x_dev), "the input was written"
    return viol.detach().clone(), x.grad.clone(), st._vg_ws


def _check_case(name, n, od, m, H, B, form, dev, seed, expect_form):
    x, w, P, stats, v64, g64, e_ref_v, e_ref_g = _inputs(n, od, m, H, B, seed)
    D = (H + 1) * n + H * m
    st = _state(P, stats, n, od, m, dev)
    plan = st.grad_plan(B, H, form)
    assert plan["form"] == expect_form and not plan["refused"], plan
    x_dev, w_dev = x.to(dev), w.to(dev)
    viol, dx, ws = _run(st, x_dev, w_dev, form)
    # it ran on the form the plan reports: the row form writes r (B, D) and nothing else; the GEMM form also leaves the
    # per-(trajectory, column block) partial sums behind it, which add up to the value
    part_off = _round64(B * D)
    if plan["form"] == "row":
        assert bool((ws[part_off:] == SENTINEL).all()), "the row form wrote past r"
    else:
        cb = plan["fwd"]["grid"][1]
        assert cb == (D + 31) // 32
        part = ws[part_off:part_off + B * cb].reshape(B, cb)
        assert not bool((part == SENTINEL).any()), "the GEMM form left no partial sums"
        assert torch.allclose(part.double().sum(dim=1), viol.double(), rtol=1e-5)
    assert not bool((ws[:B * D] == SENTINEL).any()), "no residual kept"
    # (a) value, (b) gradient
    e_v = float((viol.cpu().double() - v64).abs().max() / v64.abs().max())
    e_g = float((dx.cpu().double() - g64).abs().max() / g64.abs().max())
    print(f"\n{name}: {plan['form']} fwd grid {plan['fwd']['grid']} bwd grid {plan['bwd']['grid']}: "
          f"value e_hip {e_v:.2e} e_ref {e_ref_v:.2e}; gradient e_hip {e_g:.2e} e_ref {e_ref_g:.2e}")
    assert e_v <= _bound(e_ref_v), (e_v, e_ref_v)
    assert e_g <= _bound(e_ref_g), (e_g, e_ref_g)
    # rows with w == 0 get exactly no gradient; observation channels beyond the state get exactly 0
    zero_rows = (w == 0).nonzero().flatten().tolist()
    assert zero_rows or B < 3
    for b in zero_rows:
        assert not bool(dx[b].any())
    if od > n:
        assert not bool(dx[:, :, n:od].any())
        assert bool(dx[:, :, :n].any()) and bool(dx[:, :, od:].any())
    # (c) a second run gives the same bits
    viol2, dx2, _ = _run(st, x_dev, w_dev, form)
    assert torch.equal(viol, viol2) and torch.equal(dx, dx2)
    # (e) the row form's forward is dad_projection_violation's launch with the residual kept: the same bits
    if plan["form"] == "row":
        assert torch.equal(viol, st.violation(x_dev))
    return viol, dx, (v64, g64, e_ref_v, e_ref_g)


# (id, n, od, m, H, B, form asked for, form taken)
CASES = [
    ("row_D52_B3", 4, 4, 2, 8, 3, None, "row"),            # D < 64: one chunk
    ("row_D196_B5", 4, 4, 2, 32, 5, None, "row"),          # D % 64, D % 32 != 0; the duplicated last state
    ("row_od6", 4, 6, 2, 8, 4, None, "row"),               # od > n: the extra channels get exactly 0
    ("gemm_D52_B32", 4, 4, 2, 8, 32, "gemm", "gemm"),      # two column tiles, the last 20 wide; one K chunk, three idle waves
    ("gemm_D514_B33", 4, 4, 2, 85, 33, None, "gemm"),      # 2 row tiles, the last with 1 row; last column tile 2 wide; 9 K chunks over 4 waves
    ("gemm_D2410_B32", 4, 4, 2, 401, 32, None, "gemm"),    # the size dad_projection_violation refuses
    ("gemm_D2410_B2", 4, 4, 2, 401, 2, None, "gemm"),      #   ... with a part-filled row tile at B < 32
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_value_and_gradient_vs_float64(case, dev):
    name, n, od, m, H, B, form, expect = case
    _check_case(name, n, od, m, H, B, form, dev, seed=1000 + len(name) + 7 * B + H, expect_form=expect)


def test_row_and_gemm_forms_agree(dev):
    """row_vs_gemm_D196_B64: both forms forced on the same inputs; each within the criterion of float64, and of each
    other."""
    n, od, m, H, B = 4, 4, 2, 32, 64
    row_v, row_g, (v64, g64, e_ref_v, e_ref_g) = _check_case("row_vs_gemm_D196_B64[row]", n, od, m, H, B, "row", dev, 77, "row")
    gem_v, gem_g, _ = _check_case("row_vs_gemm_D196_B64[gemm]", n, od, m, H, B, "gemm", dev, 77, "gemm")
    d_v = float((row_v.double() - gem_v.double()).abs().max().cpu() / v64.abs().max())
    d_g = float((row_g.double() - gem_g.double()).abs().max().cpu() / g64.abs().max())
    print(f"\nrow_vs_gemm_D196_B64: |row - gemm| value {d_v:.2e}, gradient {d_g:.2e}")
    assert d_v <= _bound(e_ref_v) and d_g <= _bound(e_ref_g)


def test_a_second_graph_does_not_overwrite_the_first_ones_residual(dev):
    """Two forward passes on one state before either backward: the second takes a workspace of its own."""
    n, od, m, H, B = 4, 4, 2, 8, 3
    x, w, P, stats, v64, g64, _, e_ref_g = _inputs(n, od, m, H, B, 5)
    st = _state(P, stats, n, od, m, dev)
    with torch.enable_grad():
        xa = x.to(dev).requires_grad_(True)
        xb = (2.0 * x).to(dev).requires_grad_(True)
        va = st.violation_fn(xa)
        vb = st.violation_fn(xb)
        (vb * w.to(dev)).sum().backward()
        (va * w.to(dev)).sum().backward()
    e = float((xa.grad.cpu().double() - g64).abs().max() / g64.abs().max())
    assert e <= _bound(e_ref_g), e


def test_projection_loss_is_differentiable(dev):
    """ProjectionLoss.compute on a trajectory that requires grad: the value carries a graph, backward() fills x.grad with
    the float64 gradient of mean((v - vP)^2) — d viol / d x over B D; without grad it is the old path and bits."""
    from dynamics_aware_diffusion_amd.losses import ProjectionLoss
    n, m, H, B = 4, 2, 32, 5
    D = (H + 1) * n + H * m
    x, _, P, stats, v64, _, e_ref_v, _ = _inputs(n, n, m, H, B, 1000 + len("row_D196_B5") + 7 * B + H)
    ones = torch.ones(B)
    _, g64 = _value_and_grad(x, ones, P, n, n, stats, torch.float64)
    _, g32 = _value_and_grad(x, ones, P, n, n, stats, torch.float32)
    e_ref_g = float((g32.double() - g64).abs().max() / g64.abs().max())
    norm = cases.NormalizerStub(n, m)
    norm.obs_mean, norm.obs_std, norm.action_mean, norm.action_std = (s.numpy() for s in stats)
    pl = ProjectionLoss(P, norm, state_dim=n, action_dim=m, observation_dim=n, horizon=H, weight=0.1, device=str(dev))
    with torch.enable_grad():
        xg = x.to(dev).requires_grad_()
        value = pl.compute({"conditions": xg})
        assert value.requires_grad
        value.backward()
    torch.cuda.synchronize()
    want_v = float(v64.sum() / (B * D))
    assert abs(float(value) - want_v) <= _bound(e_ref_v) * float(v64.abs().max()) / D
    e = float((xg.grad.cpu().double() * (B * D) - g64).abs().max() / g64.abs().max())
    print(f"\nProjectionLoss.backward: e_hip {e:.2e} e_ref {e_ref_g:.2e}")
    assert e <= _bound(e_ref_g) + 2.0 ** -24          # (+ the rounding of the division by B D)
    # without grad: exactly today's path
    plain = pl.compute({"conditions": x.to(dev)})
    assert not plain.requires_grad
    assert torch.equal(plain, pl._state.violation(x.to(dev)).sum() / (B * D))
    with torch.no_grad():
        assert torch.equal(pl.compute({"conditions": xg}), plain)
    assert torch.equal(pl(({"conditions": x.to(dev)})), 0.1 * plain)


def _tiny_projection(dev, seed=9):
    od, ad, td, dim, mults = cases.net_dims("tiny")
    H = cases.H
    g = torch.Generator().manual_seed(seed)
    D = (H + 1) * od + H * ad
    P = torch.randn(D, D, generator=g) / D ** 0.5
    stats = (torch.randn(od, generator=g), 0.5 + torch.rand(od, generator=g),
             torch.randn(ad, generator=g), 0.5 + torch.rand(ad, generator=g))
    norm = cases.NormalizerStub(od, ad)
    norm.obs_mean, norm.obs_std, norm.action_mean, norm.action_std = (s.numpy() for s in stats)
    return od, ad, H, D, P, stats, norm


@pytest.mark.parametrize("pred_eps", [True, False], ids=["eps", "x0"])
def test_training_with_predicted_projection_loss(pred_eps, dev):
    """ComposedLoss([DiffusionLoss, PredictedProjectionLoss]).backward() on the tiny net (H = 32, B = 4), t and both noise
    draws injected: every parameter gradient against float64 autograd through oracle/denoiser.py and the restated
    violation, within test_hip_train's REL in units of max |g| per tensor."""
    from dynamics_aware_diffusion_amd.losses import ComposedLoss, DiffusionLoss, PredictedProjectionLoss
    from oracle import denoiser as orc
    T, B, weight = 20, 4, 0.1
    od, ad, H, D, P, stats, norm = _tiny_projection(dev)
    diff = build("tiny", T, "cosine", dev, predict_epsilon=pred_eps)
    terms = ComposedLoss([DiffusionLoss(diff, 1.0),
                          PredictedProjectionLoss(diff, P, norm, state_dim=od, action_dim=ad, observation_dim=od,
                                                  horizon=H, weight=weight, device=str(dev))])
    x0, t, noise1, _ = cases.train_inputs("vg.train.a", "tiny", T, B, False)
    _, _, noise2, _ = cases.train_inputs("vg.train.b", "tiny", T, B, False)
    tt = torch.from_numpy(t).to(dev)
    for p in diff.parameters():
        p.grad = None
    real_randint = torch.randint
    torch.randint = lambda *a, **k: tt.clone()
    try:
        with injected_noise(np.stack([noise1, noise2]), dev), torch.enable_grad():
            total, parts = terms({"conditions": torch.from_numpy(x0).to(dev)})
            assert total.requires_grad and set(parts) == {"diffusion", "predictedprojection", "total"}
            total.backward()
    finally:
        torch.randint = real_randint
    torch.cuda.synchronize()
    # float64 oracle
    w64 = {k: v.double().requires_grad_(True) for k, v in net_weights_torch("tiny").items()}
    sched = {k: v.double() for k, v in orc.schedule_buffers("cosine", T).items()}
    x64, t64 = torch.from_numpy(x0).double(), torch.from_numpy(t)
    at = lambda key: sched[key].gather(-1, t64).reshape(B, 1, 1)

    def x_t(noise):
        return at("sqrt_alphas_cumprod") * x64 + at("sqrt_one_minus_alphas_cumprod") * torch.from_numpy(noise).double()

    with torch.enable_grad():
        out1 = orc.unet_forward(w64, x_t(noise1), t64)
        l1 = ((out1 - (torch.from_numpy(noise1).double() if pred_eps else x64)) ** 2).mean()
        xt2 = x_t(noise2)
        out2 = orc.unet_forward(w64, xt2, t64)
        x0_hat = at("sqrt_recip_alphas_cumprod") * xt2 - at("sqrt_recipm1_alphas_cumprod") * out2 if pred_eps else out2
        l2 = _violation(x0_hat, P, od, od, stats).sum() / (B * D)
        (l1 + weight * l2).backward()
    assert abs(parts["diffusion"] - float(l1)) <= 5e-6 * max(1.0, abs(float(l1)))
    assert abs(parts["predictedprojection"] - weight * float(l2)) <= 2e-5 * max(1.0, abs(weight * float(l2)))
    worst, worst_key = 0.0, None
    params = dict(diff.model.named_parameters())
    assert set(params) == set(w64)
    for k, p in params.items():
        assert p.grad is not None, f"no gradient reached {k}"
        want = w64[k].grad
        e = float((p.grad.cpu().double() - want).abs().max() / max(float(want.abs().max()), 1e-12))
        if e > worst:
            worst, worst_key = e, k
        assert e <= REL, f"{k}: {e:.2e} x max|g|"
    print(f"\npredict_epsilon={pred_eps}: worst parameter-gradient error {worst:.2e} x max|g| ({worst_key}); "
          f"diffusion {float(l1):.4f}, projection term {weight * float(l2):.4f}")


def test_violation_guides_a_sampling_step(dev):
    """GuidedPolicy with guide_fn = -violation: one p_sample_with_guidance step (noise injected) against the engine's own
    step fed the float64 guide gradient.  The two differ by guide_weight * exp(log_var_t) * (g_hip - g64) — criterion (b)
    through the axpy — plus one rounding of the sum, 2^-23 of the largest |x|."""
    from dynamics_aware_diffusion_amd.guides.policies import GuidedPolicy
    from dynamics_aware_diffusion_amd.losses import ProjectionLoss
    T, B, step, gw = 20, 3, 7, 0.05
    od, ad, H, D, P, stats, norm = _tiny_projection(dev, seed=11)
    diff = build("tiny", T, "cosine", dev)
    pl = ProjectionLoss(P, norm, state_dim=od, action_dim=ad, observation_dim=od, horizon=H, device=str(dev))
    policy = GuidedPolicy(diff, norm, guide_fn=lambda x, t: -pl.violation(x), guide_weight=gw)
    x = torch.from_numpy(cases.forward_input("vg.guide.x", "tiny", B))
    noise = torch.from_numpy(cases.forward_input("vg.guide.z", "tiny", B))
    ones = torch.ones(B)
    _, g64 = _value_and_grad(x, ones, P, od, od, stats, torch.float64)
    _, g32 = _value_and_grad(x, ones, P, od, od, stats, torch.float32)
    e_ref = float((g32.double() - g64).abs().max() / g64.abs().max())
    with injected_noise(noise[None].numpy(), dev):
        got = policy.p_sample_with_guidance(x.to(dev), torch.full((B,), step, device=dev, dtype=torch.long))
    want = x.to(dev).clone()
    diff._engine(dev).denoise_step(want, step, noise=noise.to(dev), guide_grad=(-g64).float().to(dev).contiguous(), guide_weight=gw)
    torch.cuda.synchronize()
    var_t = float(diff.posterior_log_variance_clipped[step].exp())
    # (-g64).float() is itself rounded: half an ulp of max |g|
    tol = gw * var_t * (_bound(e_ref) + 2.0 ** -24) * float(g64.abs().max()) + 2.0 ** -23 * float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"\nguided step: |policy - engine(g64)| {err:.2e}, tolerance {tol:.2e}; e_ref {e_ref:.2e}")
    assert torch.isfinite(got).all() and err <= tol
    assert not torch.equal(got, x.to(dev))
