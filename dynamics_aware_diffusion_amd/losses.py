"""Loss functions — API mirror of ``m_diffuser.losses``
(/root/reference/m_diffuser/losses/__init__.py:13-236).

``DiffusionLoss`` evaluates ``GaussianDiffusion.loss`` (the denoiser runs on the HIP engine with a
per-row time embedding; differentiable through the engine's explicit backward pass);
``ProjectionLoss`` measures the dynamics violation ``mean((v - vP)^2)`` of the DATA batch in physical
units with the projection kernel of the sampler — as in the reference it depends on no parameter, so
on a data batch it contributes a value and no gradient; handed a trajectory that requires grad it is
differentiable, as the reference's plain torch expression is (``dad_projection_violation_fwd`` / ``_bwd``).
``PredictedProjectionLoss`` (not in the reference) is the same measure of the model's own predicted x_0,
the projection term that trains; ``ComposedLoss`` adds weighted terms, and
``ComposedLoss(...)(batch)[0].backward()`` is the reference's composed training step.
"""
from __future__ import annotations

import weakref
from abc import ABC, abstractmethod
from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn

from ._engine import DadError, ProjectionState


class BaseLoss(ABC, nn.Module):
    """Weighted scalar term over a batch dict with a ``'conditions'`` entry (losses:13-34)."""

    def __init__(self, weight: float = 1.0):
        super().__init__()
        self.weight = weight

    @abstractmethod
    def compute(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        ...

    def forward(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        return self.weight * self.compute(batch)


class DiffusionLoss(BaseLoss):
    """``diffusion.loss(batch['conditions'])`` (losses:37-47)."""

    def __init__(self, diffusion_model, weight: float = 1.0):
        super().__init__(weight)
        self.diffusion = diffusion_model

    def compute(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        return self.diffusion.loss(batch["conditions"])


class ProjectionLoss(BaseLoss):
    """Distance of (normalised) trajectories from the dynamics-consistent subspace, measured in
    physical units: ``mean((v - v P)^2)`` over the concatenated vector
    ``[s_0..s_{H-1}, s_{H-1}, a_0..a_{H-1}]`` (losses:50-186)."""

    def __init__(self, projection_matrix: torch.Tensor, normalizer, state_dim: int, action_dim: int,
                 observation_dim: int, horizon: int, weight: float = 0.1, device: str = "cuda"):
        super().__init__(weight)
        self.P = projection_matrix.to(device)
        self.normalizer = normalizer
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.observation_dim = observation_dim
        self.horizon = horizon
        self.device = device
        self.obs_mean = torch.from_numpy(np.asarray(normalizer.obs_mean)).float().to(device)
        self.obs_std = torch.from_numpy(np.asarray(normalizer.obs_std)).float().to(device)
        self.action_mean = torch.from_numpy(np.asarray(normalizer.action_mean)).float().to(device)
        self.action_std = torch.from_numpy(np.asarray(normalizer.action_std)).float().to(device)
        if observation_dim != state_dim:
            # the reference concatenates ALL observation channels as the state (losses:93-96,
            # 161-175), so P must have been built for n = observation_dim
            state_dim = observation_dim
        self._state = ProjectionState(self.P, self.obs_mean, self.obs_std, self.action_mean,
                                      self.action_std, state_dim, observation_dim, action_dim, device)
        self._D = (horizon + 1) * state_dim + horizon * action_dim
        if tuple(self.P.shape) != (self._D, self._D):
            raise ValueError(f"projection matrix is {tuple(self.P.shape)}, expected ({self._D}, {self._D})")

    def extract_state_actions(self, trajectory: torch.Tensor):
        return trajectory[:, :, :self.observation_dim], trajectory[:, :, self.observation_dim:]

    def unnormalize_states(self, s):
        return s * self.obs_std + self.obs_mean

    def unnormalize_actions(self, a):
        return a * self.action_std + self.action_mean

    def to_concatenated(self, state: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        ext = torch.cat([state, state[:, -1:, :]], dim=1)
        return torch.cat([ext.reshape(state.shape[0], -1), actions.reshape(actions.shape[0], -1)], dim=1)

    def violation(self, x: torch.Tensor) -> torch.Tensor:
        """``sum_d (v - vP)^2`` per trajectory, (B,), differentiable with respect to ``x`` (normalised trajectories
        (B, H, od + m)): what a guide negates, ``GuidedPolicy(..., guide_fn=lambda x, t: -loss.violation(x))``."""
        return self._state.violation_fn(x)

    def compute(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        x = batch["conditions"]
        if torch.is_grad_enabled() and x.requires_grad:
            # as the reference's plain torch expression under autograd (losses:161-186): the gradient reaches whatever
            # produced the trajectory
            return self.violation(x).sum() / (x.shape[0] * self._D)
        with torch.no_grad():
            x = x.contiguous().float()
            per_row = self._state.violation(x)                # sum_d (v - vP)^2 per trajectory
            return per_row.sum() / (x.shape[0] * self._D)


class PredictedProjectionLoss(ProjectionLoss):
    """The dynamics violation of the model's own predicted plan: ``mean((v - v P)^2)`` of ``x0_hat``, the x_0 the
    denoiser implies at a random step of the forward process.

    This term is NOT in the reference.  There, ``ProjectionLoss`` is evaluated on the data batch
    (losses/__init__.py:161-186), which depends on no parameter: it is logged and never trains anything.  What the
    project's name promises — a denoiser pushed towards plans with ``x = x P`` — needs the violation of what the model
    predicts, and its gradient with respect to the parameters; this class is that term, built from the reference's own
    pieces.  It draws ``t`` and ``noise`` as ``GaussianDiffusion.loss`` does (``torch.randint`` then
    ``torch.randn_like``; diffusion.py:253-290), forms ``x_t = q_sample(x_0, t, noise)``, evaluates
    ``out = diffusion.model(x_t, t)`` and takes ``x0_hat = out`` when the model predicts x_0, else
    ``predict_start_from_noise(x_t, t, out)`` (diffusion.py:159-166), unclamped: a clamp would cut the gradient exactly
    where the prediction is furthest off.  The value is ``mean_b violation(x0_hat_b) / D``, ``ProjectionLoss``'s
    normalisation.  It is a ``BaseLoss``, so it sits in ``ComposedLoss`` beside ``DiffusionLoss``; its draws are its
    own (a second evaluation of the denoiser per step).  With ``diffusion.fused_objective = True`` it still goes
    through the default denoiser node: the fused objective has no x0_hat output.  ``DynamicsAwareLoss`` (below) is the
    single-evaluation form of ``ComposedLoss([DiffusionLoss, PredictedProjectionLoss])``: both terms from one pair of
    draws and one evaluation of the denoiser."""

    def __init__(self, diffusion_model, projection_matrix: torch.Tensor, normalizer, state_dim: int, action_dim: int,
                 observation_dim: int, horizon: int, weight: float = 0.1, device: str = "cuda"):
        super().__init__(projection_matrix, normalizer, state_dim, action_dim, observation_dim, horizon, weight, device)
        self.diffusion = diffusion_model

    def compute(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        diff = self.diffusion
        x_start = batch["conditions"]
        diff._engine(x_start.device)              # bind schedule / options before the model call
        t = torch.randint(0, diff.n_timesteps, (x_start.shape[0],), device=x_start.device).long()
        noise = torch.randn_like(x_start)
        x_t = diff.q_sample(x_start, t, noise)
        out = diff.model(x_t, t)
        x0_hat = diff.predict_start_from_noise(x_t, t, out) if diff.predict_epsilon else out
        if torch.is_grad_enabled() and x0_hat.requires_grad:
            per_row = self.violation(x0_hat)
        else:
            per_row = self._state.violation(x0_hat.detach().contiguous().float())
        return per_row.sum() / (x_start.shape[0] * self._D)


class ComposedLoss(nn.Module):
    """Sum of weighted terms + a per-term breakdown for logging (losses:189-226)."""

    def __init__(self, losses: List[BaseLoss]):
        super().__init__()
        self.losses = nn.ModuleList(losses)

    def forward(self, batch: Dict[str, torch.Tensor]):
        total, parts = 0.0, {}
        for term in self.losses:
            value = term(batch)
            total = total + value
            parts[term.__class__.__name__.replace("Loss", "").lower()] = value.detach().item()
        parts["total"] = total.detach().item()
        return total, parts


class DynamicsAwareLoss(nn.Module):
    """The diffusion objective and the dynamics violation of the predicted plan from ONE evaluation of the denoiser:
    ``total = diffusion_weight * Ld + projection_weight * Lp``.

    Called on a batch dict.  It makes one pair of draws, in ``GaussianDiffusion.loss``'s order on
    ``batch["conditions"]``'s device (``torch.randint`` then ``torch.randn_like``), forms ``x_t = q_sample(x0, t, noise)``
    and evaluates ``out = diffusion.model(x_t, t)`` once.  ``Ld`` is exactly ``GaussianDiffusion.loss``'s term (L1 / L2
    against the noise or x_0, ``batch["weights"]`` if present, mean).  ``Lp = sum_b tw[t_b] violation(x0_hat_b) / (B D)``
    with ``x0_hat = predict_start_from_noise(x_t, t, out)`` under ``predict_epsilon``, else ``out``; unclamped, as in
    ``PredictedProjectionLoss``.  ``timestep_weights`` (``tw``): a ``(len(betas),)`` tensor, or None for all ones — it
    keeps the term off the steps where ``sqrt_recipm1_alphas_cumprod`` is in the hundreds.

    Returns ``(total, parts)``; ``parts["diffusion"]`` is the UNWEIGHTED ``Ld``, ``parts["projection"]`` the WEIGHTED
    ``projection_weight * Lp`` and ``parts["total"]`` the total, floats fetched with one device-to-host copy.  It drops
    into ``Trainer(loss_fn=..., loss_names=["diffusion", "projection", "total"])``.

    Two routes, see :meth:`route`: "default" composes the existing autograd nodes (the denoiser's, torch ops,
    ``ProjectionState.violation_fn``); "library" is one autograd node over dad_train_dynamics_objective_forward /
    _backward (opt-in through ``diffusion.fused_objective``).  Neither gives the projector a gradient; the library
    route gives x_0 none (a trajectory that requires grad takes the default route)."""

    def __init__(self, diffusion_model, projection_matrix: torch.Tensor, normalizer, state_dim: int, action_dim: int,
                 observation_dim: int, horizon: int, projection_weight: float = 0.1, diffusion_weight: float = 1.0,
                 timestep_weights=None, device: str = "cuda"):
        super().__init__()
        n = observation_dim            # (as ProjectionLoss: all observation channels are the state)
        D = (horizon + 1) * n + horizon * action_dim
        if tuple(projection_matrix.shape) != (D, D):
            raise ValueError(f"projection matrix is {tuple(projection_matrix.shape)}, expected ({D}, {D})")
        timestep_weights = self._checked_timestep_weights(diffusion_model, timestep_weights)
        # (ProjectionLoss's constructor: the projector's device state and the normaliser statistics)
        self._projection = ProjectionLoss(projection_matrix, normalizer, state_dim, action_dim, observation_dim, horizon,
                                          projection_weight, device)
        self._setup(diffusion_model, self._projection._state, D, horizon, projection_weight, diffusion_weight)
        self.timestep_weights = None if timestep_weights is None else timestep_weights.to(device)

    @staticmethod
    def _checked_timestep_weights(diffusion_model, timestep_weights):
        if timestep_weights is None:
            return None
        n_steps = int(diffusion_model.betas.shape[0])
        timestep_weights = torch.as_tensor(timestep_weights, dtype=torch.float32).detach().contiguous()
        if tuple(timestep_weights.shape) != (n_steps,):
            raise ValueError(f"timestep_weights is {tuple(timestep_weights.shape)}, expected ({n_steps},)")
        return timestep_weights

    def _setup(self, diffusion_model, state, D, horizon, projection_weight, diffusion_weight):
        self.diffusion = diffusion_model
        self._state, self._D, self.horizon = state, D, horizon
        self.projection_weight = float(projection_weight)
        self.diffusion_weight = float(diffusion_weight)
        self.timestep_weights = None
        self.form = None              # test hook: "row" / "gemm" force the violation kernels' form on either route
        self.last_route = None        # the route the last call took

    @classmethod
    def host(cls, diffusion_model, state_dim: int, action_dim: int, observation_dim: int, horizon: int,
             projection_weight: float = 0.1, diffusion_weight: float = 1.0) -> "DynamicsAwareLoss":
        """A loss without a projector or a device: enough for :meth:`route` (as ``ProjectionState.host`` plans)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        D = (horizon + 1) * observation_dim + horizon * action_dim
        self._setup(diffusion_model, ProjectionState.host(observation_dim, observation_dim, action_dim), D, horizon,
                    projection_weight, diffusion_weight)
        return self

    def _plan_engine(self):
        """The engine whose planner :meth:`route` asks (the one a call would train through)."""
        return self.diffusion.model.engine(self.horizon, self._state.device, training=True)

    def _plain_loss(self):
        fn = self.diffusion.loss_fn
        kind = "l1" if type(fn) is nn.L1Loss else "l2" if type(fn) is nn.MSELoss else None
        return kind if kind is not None and getattr(fn, "reduction", None) == "none" else None

    def route(self, batch_size: int, x0: torch.Tensor = None):
        """``("library" | "default", why)``: the route a call on ``batch_size`` trajectories (``x0``, when given: this
        batch) takes.  Library only when ``diffusion.fused_objective`` is on, the loss is the constructor's plain L1 /
        L2, x_0 does not require grad and the planner accepts the shape; everything else takes the default route."""
        diff = self.diffusion
        if not diff.fused_objective:
            return "default", "fused_objective is off"
        if self._plain_loss() is None:
            return "default", "loss_fn is not the plain L1 / L2 the library knows"
        if x0 is not None and torch.is_grad_enabled() and x0.requires_grad:
            return "default", "x_0 requires grad"
        return self._planned_route(int(batch_size))

    def _planned_route(self, batch_size: int):
        """The planner's half of :meth:`route`, asked once per (engine, batch size, form): a training loop calls
        :meth:`route` every step."""
        eng = self._plan_engine()
        held = self.__dict__.get("_route_cache")
        if held is None or held[0]() is not eng:
            held = self.__dict__["_route_cache"] = (weakref.ref(eng), {})
        key = (batch_size, self.form)
        if key not in held[1]:
            held[1][key] = self._ask_planner(eng, batch_size)
        return held[1][key]

    def _ask_planner(self, eng, batch_size: int):
        try:
            plan = eng.dynamics_objective_plan(batch_size, state=self._state, form=self.form)
        except DadError as e:              # the planner's refusal, with its message; anything else is a bug and raises
            return "default", f"planner: {e}"
        if plan["refused"]:
            return "default", "planner: the forced row form exceeds one CU's LDS"
        if plan["D"] != self._D:
            return "default", f"planner: D={plan['D']} for the model's horizon, the projector has {self._D}"
        return "library", f"one node, {plan['form']} form"

    def forward(self, batch: Dict[str, torch.Tensor]):
        diff = self.diffusion
        x0 = batch["conditions"]
        weights = batch.get("weights") if hasattr(batch, "get") else None
        B = x0.shape[0]
        diff._engine(x0.device)                   # bind schedule / options before the model call
        t = torch.randint(0, diff.n_timesteps, (B,), device=x0.device).long()
        noise = torch.randn_like(x0)
        self.last_route = self.route(B, x0)[0]
        if self.last_route == "library":
            parts = diff.model.dynamics_objective(
                x0, t, noise, weights, self._plain_loss(), diff.sqrt_alphas_cumprod, diff.sqrt_one_minus_alphas_cumprod,
                self._state, self.form, self.diffusion_weight, self.projection_weight, self.timestep_weights)
            total = parts[2]
        else:
            x_t = diff.q_sample(x0, t, noise)
            out = diff.model(x_t, t)
            loss = diff.loss_fn(out, noise if diff.predict_epsilon else x0)
            if weights is not None:
                loss = loss * weights
            ld = loss.mean()
            x0_hat = diff.predict_start_from_noise(x_t, t, out) if diff.predict_epsilon else out
            state = self._state
            if torch.is_grad_enabled() and x0_hat.requires_grad:
                per_row = state.violation_fn(x0_hat, self.form)
            else:
                per_row = state.violation(x0_hat.detach().contiguous().float())
            if self.timestep_weights is not None:
                per_row = per_row * self.timestep_weights[t]
            lp = self.projection_weight * (per_row.sum() / (B * self._D))
            total = self.diffusion_weight * ld + lp
            parts = torch.stack([ld.detach(), lp.detach(), total.detach()])
        d, p, tot = parts.detach().tolist()       # one device-to-host copy
        return total, {"diffusion": d, "projection": p, "total": tot}


__all__ = ["BaseLoss", "DiffusionLoss", "ProjectionLoss", "PredictedProjectionLoss", "ComposedLoss", "DynamicsAwareLoss"]
