"""``GaussianDiffusion`` — API mirror of ``m_diffuser.models.diffusion.GaussianDiffusion``
(/root/reference/m_diffuser/models/diffusion.py:51-294) for the sampling path.

Schedules are computed with the same fp32 torch ops, in the same order, as the reference
(diffusion.py:32-48, 104-128), so the 12 registered buffers are bit-identical and a
reference checkpoint's buffers load unchanged.  ``p_mean_variance`` / ``p_sample`` /
``p_sample_loop`` run on the HIP engine; the per-step tail (x0 prediction, clamp, posterior
mean, noise, inpainting) is one fused kernel behind ``dad_denoise_step``.  ``loss`` evaluates the
training objective on the same kernels and is differentiable (explicit backward pass of the engine).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .temporal_unet import TemporalUnet

_ENGINE_BUFFERS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                   "posterior_mean_coef1", "posterior_mean_coef2",
                   "posterior_log_variance_clipped")


def cosine_beta_schedule(timesteps: int, s: float = 0.008) -> torch.Tensor:
    """Nichol & Dhariwal cosine schedule, clipped to [1e-4, 0.9999] (diffusion.py:32-41)."""
    grid = torch.linspace(0, timesteps, timesteps + 1)
    abar = torch.cos(((grid / timesteps) + s) / (1 + s) * torch.pi * 0.5) ** 2
    abar = abar / abar[0]
    return torch.clip(1 - (abar[1:] / abar[:-1]), 0.0001, 0.9999)


def linear_beta_schedule(timesteps: int, beta_start: float = 1e-4,
                         beta_end: float = 0.02) -> torch.Tensor:
    """DDPM linear schedule (diffusion.py:44-48)."""
    return torch.linspace(beta_start, beta_end, timesteps)


def make_schedule(beta_schedule: str, n_timesteps: int) -> Dict[str, torch.Tensor]:
    """All 12 schedule buffers, in registration order (diffusion.py:96-128)."""
    if beta_schedule == "linear":
        betas = linear_beta_schedule(n_timesteps)
    elif beta_schedule == "cosine":
        betas = cosine_beta_schedule(n_timesteps)
    else:
        raise ValueError(f"Unknown beta schedule: {beta_schedule}")
    alphas = 1.0 - betas
    abar = torch.cumprod(alphas, dim=0)
    abar_prev = torch.cat([torch.ones(1), abar[:-1]])
    post_var = betas * (1.0 - abar_prev) / (1.0 - abar)
    bufs = {"betas": betas, "alphas": alphas, "alphas_cumprod": abar,
            "alphas_cumprod_prev": abar_prev}
    bufs["sqrt_alphas_cumprod"] = torch.sqrt(abar)
    bufs["sqrt_one_minus_alphas_cumprod"] = torch.sqrt(1.0 - abar)
    bufs["sqrt_recip_alphas_cumprod"] = torch.sqrt(1.0 / abar)
    bufs["sqrt_recipm1_alphas_cumprod"] = torch.sqrt(1.0 / abar - 1)
    bufs["posterior_variance"] = post_var
    bufs["posterior_log_variance_clipped"] = torch.log(torch.clamp(post_var, min=1e-20))
    bufs["posterior_mean_coef1"] = betas * torch.sqrt(abar_prev) / (1.0 - abar)
    bufs["posterior_mean_coef2"] = (1.0 - abar_prev) * torch.sqrt(alphas) / (1.0 - abar)
    return bufs


def extract(a: torch.Tensor, t: torch.Tensor, x_shape: tuple) -> torch.Tensor:
    """Per-row schedule lookup broadcastable to ``x_shape`` (diffusion.py:15-29); raises
    ``RuntimeError`` when ``t`` exceeds the schedule, like the reference's gather."""
    picked = a.gather(-1, t)
    return picked.reshape(t.shape[0], *((1,) * (len(x_shape) - 1)))


def sampler_timesteps(n_trained: int, timesteps_or_K) -> np.ndarray:
    """The strictly ascending timesteps ``tau`` of a strided sampler over a trained schedule of ``n_trained`` entries:
    ``K`` (an int, 1 <= K <= n_trained) means ``tau_i = floor(i * n_trained / K)``; a sequence is taken as given.
    ``ValueError`` for K out of range and for a sequence that is empty, unsorted, repeated or out of [0, n_trained)."""
    T = int(n_trained)
    if isinstance(timesteps_or_K, (int, np.integer)) and not isinstance(timesteps_or_K, bool):
        K = int(timesteps_or_K)
        if K < 1 or K > T:
            raise ValueError(f"steps = {K} is outside [1, {T}], the trained schedule")
        return (np.arange(K, dtype=np.int64) * T) // K
    try:
        given = [v for v in timesteps_or_K]
    except TypeError:
        raise ValueError(f"steps must be an int or a sequence of timesteps, got {timesteps_or_K!r}") from None
    if not given or any(isinstance(v, bool) or int(v) != v for v in given):
        raise ValueError("a sampler's timesteps must be a non-empty sequence of integers")
    tau = np.asarray([int(v) for v in given], dtype=np.int64)
    if tau.min() < 0 or tau.max() >= T:
        raise ValueError(f"a sampler's timesteps must lie in [0, {T})")
    if np.any(np.diff(tau) <= 0):
        raise ValueError("a sampler's timesteps must be strictly ascending (no repeats)")
    return tau


def ddim_table(alphas_cumprod, timesteps_or_K, eta: float = 0.0) -> Dict[str, np.ndarray]:
    """Coefficients of the strided (DDIM, Song et al. 2021) sampler over a trained schedule; needs no device.

    ``alphas_cumprod`` is the model's buffer, read as float64; ``timesteps_or_K`` as ``sampler_timesteps``; ``eta`` in
    [0, 1] (0: deterministic, 1: the ancestral variance).  Step ``i`` goes from ``ab = abar[tau_i]`` to
    ``ap = abar[tau_{i-1}]`` (``ap = 1`` for i = 0)::

        sigma      = eta * sqrt((1 - ap) / (1 - ab)) * sqrt(1 - ab / ap)
        c          = sqrt(max(1 - ap - sigma^2, 0)) / sqrt(1 - ab)
        coef_xt    = c
        coef_x0    = sqrt(ap) - c * sqrt(ab)
        c_recip    = sqrt(1 / ab)
        c_recipm1  = sqrt(1 / ab - 1)
        guide_x0   = (1 - ab) / sqrt(ab)
        guide_mean = 0

    so that ``mean = coef_x0 * x0 + coef_xt * x_t`` is ``sqrt(ap) x0 + sqrt(1 - ap - sigma^2) eps`` with eps re-derived
    from the (clamped) x0, and ``guide_x0`` is the shift of x0 that ``eps' = eps - w sqrt(1 - ab) g`` causes.  Returns
    ``tau`` (int64) and one float64 array per name above, index i; ``_engine.pack_sampler_steps`` rounds them to fp32,
    once.  ``eta = 1`` with every timestep is the DDPM posterior (coef1, coef2, variance) of the same ``abar``."""
    if torch.is_tensor(alphas_cumprod):
        alphas_cumprod = alphas_cumprod.detach().to("cpu")
        abar = alphas_cumprod.to(torch.float64).numpy()
    else:
        abar = np.asarray(alphas_cumprod, dtype=np.float64)
    if abar.ndim != 1 or abar.shape[0] < 1:
        raise ValueError("alphas_cumprod must be a non-empty vector")
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:                      # (NaN fails both comparisons)
        raise ValueError(f"eta = {eta} is outside [0, 1]")
    tau = sampler_timesteps(abar.shape[0], timesteps_or_K)
    ab = abar[tau]
    ap = np.concatenate([np.ones(1), ab[:-1]])
    sigma = eta * np.sqrt((1.0 - ap) / (1.0 - ab)) * np.sqrt(np.maximum(1.0 - ab / ap, 0.0))
    c = np.sqrt(np.maximum(1.0 - ap - sigma * sigma, 0.0)) / np.sqrt(1.0 - ab)
    return {"tau": tau, "c_recip": np.sqrt(1.0 / ab), "c_recipm1": np.sqrt(1.0 / ab - 1.0),
            "guide_x0": (1.0 - ab) / np.sqrt(ab), "coef_x0": np.sqrt(ap) - c * np.sqrt(ab), "coef_xt": c,
            "guide_mean": np.zeros_like(ab), "sigma": sigma}


class _LoopSteps:
    """The steps one sampling loop runs, in execution order: all that differs between the samplers.

    ``timesteps[j]`` is the timestep of iteration j; ``takes_noise`` says whether an iteration consumes a z;
    ``step(eng, x, j, **kw)`` runs iteration j alone; ``loop(eng, x, alphas, **kw)`` runs all of them as the fused
    engine loop, ``alphas`` being ``None`` or one projection strength per iteration."""

    def __init__(self, timesteps, takes_noise, step, loop):
        self.timesteps, self.takes_noise, self.step, self.loop = timesteps, takes_noise, step, loop

    @classmethod
    def ancestral(cls, n_steps: int, n_trained: int) -> "_LoopSteps":
        """t = n_steps-1 .. 0 over the first ``n_steps`` of ``n_trained`` schedule entries; the library holds the
        coefficients (dad_denoise_step / dad_sample_loop)."""
        timesteps = list(reversed(range(n_steps)))

        def step(eng, x, j, **kw):
            eng.denoise_step(x, timesteps[j], **kw)

        def loop(eng, x, alphas, **kw):
            table = None
            if alphas is not None:                 # dad_sample_loop reads its strengths by timestep, not by iteration
                table = [0.0] * n_trained
                for t, a in zip(timesteps, alphas):
                    table[t] = a
            eng.sample_loop(x, n_steps, proj_alphas=table, **kw)

        return cls(timesteps, True, step, loop)

    @classmethod
    def strided(cls, plan) -> "_LoopSteps":
        """The steps of ``GaussianDiffusion.sampler_plan()``, given by their coefficients (dad_sampler_step /
        dad_sampler_loop); ``eta == 0`` makes sigma 0 at every step, so x_T is the only draw."""
        steps, taus, eta = plan

        def step(eng, x, j, **kw):
            eng.sampler_step(x, steps[j], **kw)

        def loop(eng, x, alphas, **kw):
            eng.sampler_loop(x, steps, proj_alphas=alphas, **kw)

        return cls(taus, eta > 0.0, step, loop)


class GaussianDiffusion(nn.Module):
    """DDPM over trajectories (batch, horizon, observation_dim + action_dim).

    Constructor, attributes (``horizon``, ``observation_dim``, ``action_dim``,
    ``transition_dim``, mutable ``n_timesteps``, ``betas`` ...) and method names follow the
    reference (diffusion.py:62-136) because ``scripts/evaluate.py`` and the policies read
    them directly.  Extra, build-specific knob: ``sampler_rng``:

    * ``"torch"`` (default) draws x_T and every z with ``torch.randn`` in the reference's call
      order (diffusion.py:241,218), so a seeded run consumes the device generator exactly
      like the reference would on the same device;
    * ``"philox"`` uses the engine's in-kernel counter-based generator (no noise tensors,
      sharding-invariant) — the throughput path.

    ``use_graph = True`` replays the whole T-step loop as one cached hipGraph (persistent
    input buffers, result returned as a copy): removes the per-launch host cost that dominates
    small batches such as the B=1 plans of ``get_action``.

    ``set_sampler("ddim", steps=K, eta=0.0)`` makes every loop (``p_sample_loop``, the policies' ``sample_loop`` and
    what is built on it) a K-step strided sampler over the whole trained schedule, on the same fused loop; the
    default, ``"ddpm"``, is the reference's ancestral loop over the first ``n_timesteps`` entries.
    """

    def __init__(self, model: TemporalUnet, horizon: int, observation_dim: int, action_dim: int,
                 n_timesteps: int = 1000, loss_type: str = "l2", clip_denoised: bool = True,
                 predict_epsilon: bool = True, beta_schedule: str = "cosine"):
        super().__init__()
        self.model = model
        self.horizon = horizon
        self.observation_dim = observation_dim
        self.action_dim = action_dim
        self.transition_dim = observation_dim + action_dim
        self.n_timesteps = n_timesteps
        self.clip_denoised = clip_denoised
        self.predict_epsilon = predict_epsilon
        self.beta_schedule = beta_schedule
        for name, buf in make_schedule(beta_schedule, n_timesteps).items():
            self.register_buffer(name, buf)
        if loss_type == "l1":
            self.loss_fn = nn.L1Loss(reduction="none")
        elif loss_type == "l2":
            self.loss_fn = nn.MSELoss(reduction="none")
        else:
            raise ValueError(f"Unknown loss type: {loss_type}")
        self.sampler_rng = "torch"
        self.seed = 0
        self.use_graph = False
        # "torch" RNG: the fused loop takes the whole z stack (T, B, H, td) up to this many bytes;
        # beyond it z is drawn step by step (same draws, same order, O(1) memory in T)
        self.max_noise_stack_bytes = 256 << 20
        # True: ``loss`` runs q_sample, the time MLPs, the denoiser and the L1 / L2 mean inside the library, as one
        # autograd node over the parameters (dad_train_objective_forward / _backward).  Opt-in; False changes nothing.
        self.fused_objective = False
        # ("ddpm", None, 0.0) or ("ddim", (tau_0, ..., tau_{K-1}), eta): plain data, see set_sampler
        self.sampler = ("ddpm", None, 0.0)

    def set_sampler(self, kind: str, steps: Union[None, int, Sequence[int]] = None, eta: float = 0.0) -> None:
        """Choose what the sampling loops run.

        ``"ddpm"`` (the default; takes no arguments): the ancestral loop t = n_timesteps-1 .. 0 of the reference.
        ``"ddim"``: the strided sampler of ``ddim_table`` over the whole trained schedule (``len(betas)`` entries,
        whatever ``n_timesteps`` was lowered to): ``steps`` is K (``tau_i = floor(i T / K)``) or an explicit strictly
        ascending sequence of timesteps, ``eta`` in [0, 1] scales the per-step noise (0: deterministic given x_T).

        The choice is a plain attribute (``state_dict`` does not carry it; ``deepcopy`` and pickle do); the engine is
        neither rebuilt nor re-finalised, the coefficients travel with each call.  The single-step methods
        (``p_sample``, ``p_mean_variance``, the policies' ``p_sample_with_guidance``) stay ancestral steps."""
        if kind == "ddpm":
            if steps is not None or eta != 0.0:
                raise ValueError("the ancestral sampler takes no steps and no eta: lower n_timesteps to truncate it")
            self.sampler = ("ddpm", None, 0.0)
            return
        if kind != "ddim":
            raise ValueError(f"unknown sampler {kind!r} (\"ddpm\" or \"ddim\")")
        if steps is None:
            raise ValueError("the strided sampler needs steps: K or a sequence of timesteps")
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta = {eta} is outside [0, 1]")
        tau = sampler_timesteps(int(self.betas.shape[0]), steps)
        self.sampler = ("ddim", tuple(int(v) for v in tau), eta)

    def sampler_plan(self):
        """``None`` for the ancestral sampler; else ``(steps, tau, eta)`` of the strided one in EXECUTION order
        (i = K-1 .. 0): the engine's coefficient array, the timesteps the network sees, the noise scale."""
        kind, tau, eta = getattr(self, "sampler", ("ddpm", None, 0.0))
        if kind == "ddpm":
            return None
        # computed once per (sampler, schedule buffer): reading ``alphas_cumprod`` back is a device-to-host copy, which
        # would otherwise drain the stream at the start of every loop (plain numpy data: deepcopy and pickle carry it)
        abar = self.alphas_cumprod
        key = (kind, tau, eta, abar.data_ptr(), abar._version, str(abar.device))
        cached = self.__dict__.get("_sampler_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        from .._engine import pack_sampler_steps
        table = ddim_table(abar, tau, eta)
        order = np.arange(len(tau))[::-1]
        plan = (pack_sampler_steps(table, order), [int(tau[i]) for i in order], eta)
        self.__dict__["_sampler_cache"] = (key, plan)
        return plan

    @staticmethod
    def noise_stack_bytes(shape, n_steps: int) -> int:
        n = 4 * int(n_steps)
        for d in shape:
            n *= int(d)
        return n

    # ------------------------------------------------------------------ engine access
    def _engine(self, device: torch.device):
        sched = {k: getattr(self, k) for k in _ENGINE_BUFFERS}
        self.model.bind_diffusion(sched, int(self.betas.shape[0]), self.predict_epsilon,
                                  self.clip_denoised)
        return self.model.engine(self.horizon, device)

    def _check_step(self, t: int) -> None:
        if t < 0 or t >= int(self.betas.shape[0]):
            # reference: RuntimeError raised by gather in extract() (diffusion.py:28)
            raise RuntimeError(f"index {t} is out of bounds for dimension 0 with size "
                               f"{int(self.betas.shape[0])}")

    # ------------------------------------------------------------------ closed forms
    def q_sample(self, x_start: torch.Tensor, t: torch.Tensor,
                 noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q(x_t | x_0) (diffusion.py:138-157)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        return (extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def predict_start_from_noise(self, x_t, t, noise):
        """x0 = sqrt(1/abar_t) x_t - sqrt(1/abar_t - 1) eps (diffusion.py:159-166)."""
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                - extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)

    def q_posterior(self, x_start, x_t, t) -> Tuple[torch.Tensor, torch.Tensor]:
        """(posterior mean, clipped log variance) (diffusion.py:168-180)."""
        mean = (extract(self.posterior_mean_coef1, t, x_t.shape) * x_start
                + extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        return mean, extract(self.posterior_log_variance_clipped, t, x_t.shape)

    # ------------------------------------------------------------------ reverse process
    @torch.no_grad()
    def p_mean_variance(self, x: torch.Tensor, t: Union[int, torch.Tensor]
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(model mean, (B,1,1) log variance) of p(x_{t-1} | x_t) (diffusion.py:182-203): the reference's ancestral
        step, whatever ``set_sampler`` chose for the loops."""
        step = TemporalUnet.shared_timestep(t)
        self._check_step(step)
        eng = self._engine(x.device)
        xc = x.contiguous().float()
        mean = torch.empty_like(xc)
        eng.denoise_step(xc, step, mean_out=mean, update_x=False)
        logvar = self.posterior_log_variance_clipped[step].reshape(1, 1, 1).expand(
            x.shape[0], 1, 1)
        return mean, logvar

    @torch.no_grad()
    def p_sample(self, x: torch.Tensor, t: Union[int, torch.Tensor]) -> torch.Tensor:
        """x_{t-1} ~ p(. | x_t); z is drawn even at t == 0 and masked (diffusion.py:205-223): the reference's
        ancestral step, whatever ``set_sampler`` chose for the loops."""
        step = TemporalUnet.shared_timestep(t)
        self._check_step(step)
        eng = self._engine(x.device)
        out = x.contiguous().float().clone()
        noise = torch.randn_like(out)
        eng.denoise_step(out, step, noise=noise)
        return out

    @torch.no_grad()
    def p_sample_loop(self, shape: tuple, verbose: bool = False, row_offset: int = 0
                      ) -> torch.Tensor:
        """Full ancestral sampling t = n_timesteps-1 .. 0 from pure noise (diffusion.py:225-251).

        ``n_timesteps`` may have been lowered after construction (evaluate.py:350-353): the
        loop then walks the first ``n_timesteps`` entries of the trained schedule.  Under
        ``set_sampler("ddim", ...)`` it is the K-step strided loop over the whole trained schedule instead.
        """
        return self._reverse_loop(self._engine(self.betas.device), tuple(shape), row_offset)

    def _loop_steps(self) -> "_LoopSteps":
        """What ``set_sampler`` chose, as the steps a loop runs."""
        plan = self.sampler_plan()
        if plan is not None:
            return _LoopSteps.strided(plan)
        self._check_step(int(self.n_timesteps) - 1)
        return _LoopSteps.ancestral(int(self.n_timesteps), int(self.betas.shape[0]))

    def _reverse_loop(self, eng, shape: tuple, row_offset: int, cond0: Optional[torch.Tensor] = None,
                      rest: Optional[Dict[int, torch.Tensor]] = None, guide=None, guide_weight: float = 0.0,
                      projector=None, alpha_of=None, library_guide=None) -> torch.Tensor:
        """Every sampling loop: x_T ~ N(0, I), the conditions, then the reverse steps of ``_loop_steps`` by the one
        route the settings allow.  ``p_sample_loop`` is this with nothing but a shape; the policies' ``sample_loop``
        adds the rest.

        ``cond0`` / ``rest``: the condition at horizon step 0 (the engine inpaints it inside every step) and those
        at other steps ``{k: value}`` (written with torch indexing after each step), on the device as float32.
        ``guide(x, t_tensor) -> grad`` with its ``guide_weight``: the guide's gradient at x_t, fused into the step
        (the ancestral step scales it by the variance; the strided one takes classifier guidance in its DDIM form,
        eps' = eps - w sqrt(1 - abar) g, as the shift of x0 it causes).  ``projector.apply(x, alpha_of(t))`` follows
        the step at timestep t.  ``library_guide``: the same guide as a ``GuideState`` the library evaluates inside
        the fused loop (dad_guided_loop); with it a guided loop without ``rest`` is one engine call, and ``guide`` is
        not called.

        Philox: x_T is draw 0 and iteration j's z is draw j + 1 of (``seed``, ``row_offset`` + row).  torch: x_T is
        the first ``randn`` and iteration j's z the next one after it, in the reference's call order
        (diffusion.py:241,218); a loop whose steps take no noise draws nothing after x_T."""
        device = self.betas.device
        steps = self._loop_steps()
        n, rest = len(steps.timesteps), rest or {}
        philox = self.sampler_rng == "philox"
        # the fused engine loop knows no guide but a library guide and no condition beyond horizon step 0.  Only it
        # replays a graph, which needs persistent (address-stable) buffers and hands the result out as a copy: decided
        # before any allocation
        if guide is None or not guide_weight > 0:
            library_guide = None
        fused = (guide is None or library_guide is not None) and not rest
        graph = bool(self.use_graph) and fused
        if philox:
            x = eng.persistent("x", shape) if graph else torch.empty(shape, device=device, dtype=torch.float32)
            eng.fill_normal(x, self.seed, row_offset=row_offset, draw=0)
        else:
            x = torch.randn(shape, device=device)
            if graph:
                x = eng.persistent("x", shape).copy_(x)
        if cond0 is not None:
            x[:, 0] = cond0
            cond0 = cond0.contiguous()
            if graph:                                          # frozen pointer: stage the condition
                cond0 = eng.persistent("cond0", tuple(cond0.shape)).copy_(cond0)
        for k, v in rest.items():
            x[:, k] = v
        alphas = None if projector is None else [alpha_of(t) for t in steps.timesteps]

        if fused:
            kw = dict(cond0=cond0, projection=projector, use_graph=graph)
            if library_guide is not None:          # (extra keywords only here: an engine without the guide never sees them)
                kw.update(guide=library_guide, guide_weight=float(guide_weight))
            if philox:
                steps.loop(eng, x, alphas, seed=self.seed, row_offset=row_offset, **kw)
            elif steps.takes_noise and self.noise_stack_bytes(shape, n) > self.max_noise_stack_bytes:
                # the whole z stack would not be O(1) in T (1.1 GB for Door at B=128, T=1000): draw z step by step
                # instead: the same torch.randn calls in the same order, one engine step per iteration
                for j in range(n):
                    gkw = {}
                    if library_guide is not None:
                        gkw = dict(guide_grad=library_guide.grad(x), guide_weight=float(guide_weight))
                    steps.step(eng, x, j, noise=torch.randn(shape, device=device), cond0=cond0, **gkw)
                    if projector is not None:
                        projector.apply(x, alphas[j])
            else:
                stack = None
                if steps.takes_noise:
                    stack = eng.persistent("z", (n,) + shape) if graph else torch.empty((n,) + shape, device=device)
                    for j in range(n):
                        torch.randn(shape, out=stack[j])
                # (no stack and no seed: nothing is drawn, the loop's default Philox stream is never read)
                steps.loop(eng, x, alphas, noise_stack=stack, **kw)
            return x.clone() if graph else x

        # guided (or multi-step-conditioned) route: one engine step per iteration, the guide gradient comes from
        # PyTorch autograd on the user's value model.
        for j, t in enumerate(steps.timesteps):
            grad, gw = None, 0.0
            if guide is not None:
                grad = guide(x, torch.full((shape[0],), t, device=device, dtype=torch.long)).float()
                gw = float(guide_weight)
            if philox or not steps.takes_noise:
                steps.step(eng, x, j, seed=self.seed, row_offset=row_offset, draw=j + 1, cond0=cond0,
                           guide_grad=grad, guide_weight=gw)
            else:
                steps.step(eng, x, j, noise=torch.randn_like(x), cond0=cond0, guide_grad=grad, guide_weight=gw)
            for k, v in rest.items():
                x[:, k] = v
            if projector is not None:
                projector.apply(x, alphas[j])
        return x

    # ------------------------------------------------------------------ training objective
    def loss(self, x_start: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The diffusion training objective (diffusion.py:253-290): t ~ randint per trajectory,
        noise ~ randn, x_t = q_sample, denoiser on the HIP engine (per-row time embedding),
        elementwise L1 / L2 against the noise (or x_0), optional weights, mean.

        Same random draws in the same order as the reference (``torch.randint`` then
        ``torch.randn_like`` on ``x_start``'s device).  With gradients enabled the result carries an
        autograd graph whose denoiser node is the engine's explicit backward pass
        (``dad_unet_backward``): ``loss.backward()`` fills ``.grad`` of every parameter, as the
        reference's training step expects (utils/training.py:152-156).  Under ``torch.no_grad()`` it
        is the forward-only validation loss.

        ``fused_objective = True`` (opt-in) keeps the two draws here and hands everything after them to the library:
        the result is the scalar of one autograd node whose inputs are the parameters, the time MLPs included.  A
        trajectory that itself requires grad takes the path above."""
        batch = x_start.shape[0]
        self._engine(x_start.device)              # bind schedule / options before the model call
        t = torch.randint(0, self.n_timesteps, (batch,), device=x_start.device).long()
        noise = torch.randn_like(x_start)
        # (the library knows the two elementwise losses the constructor builds; a replaced loss_fn runs as it is, below)
        fused_loss = "l1" if type(self.loss_fn) is nn.L1Loss else "l2" if type(self.loss_fn) is nn.MSELoss else None
        if fused_loss is not None and getattr(self.loss_fn, "reduction", None) != "none":
            fused_loss = None
        if self.fused_objective and fused_loss is not None and not (torch.is_grad_enabled() and x_start.requires_grad):
            return self.model.objective(x_start, t, noise, weights, fused_loss,
                                        self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)
        x_noisy = self.q_sample(x_start, t, noise)
        model_output = self.model(x_noisy, t)
        target = noise if self.predict_epsilon else x_start
        loss = self.loss_fn(model_output, target)
        if weights is not None:
            loss = loss * weights
        return loss.mean()

    def forward(self, x, *args, **kwargs):
        return self.loss(x, *args, **kwargs)
