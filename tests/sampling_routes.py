"""The route table of the sampling loops, walked on the CPU against recording stubs (no library, no device).

``CASES`` is the product sampler x sampler_rng x use_graph x max_noise_stack_bytes x entry point; ``run_case`` runs one
of them and returns its trace, a list of short strings.  ``tests/golden/make_sampling_routes.py`` wrote the traces of
the drivers as they were before the four copies of the decision tree became one (``sampling_routes.json``), and
``test_sampling_routes_host.py`` holds every later driver to them.

What a trace holds is what the library or the caller can observe: the engine calls in order with their arguments (a
content hash stands for a tensor, so the hash of ``z`` says which ``torch.randn`` draw it was), the projection
strengths in execution order, on the fused loop which of ``x`` / ``noise_stack`` / ``cond0`` are persistent buffers (the
pointers a graph freezes), the next draw of the generator after the call, and the result.  The stubs change ``x`` from
all their arguments, so an exchanged pair of steps, conditions or projections changes every hash after it.  Where
``persistent()`` is asked for on a route that replays no graph is not recorded.

The arithmetic of the stubs is elementwise fp32 (IEEE, the same everywhere); ``torch.randn`` itself is the same on
every CPU that takes torch's vectorised path (AVX2 and up), which is where the fixture was written.
"""
from __future__ import annotations

import hashlib
import itertools
import types

import numpy as np
import torch

B, HORIZON, OBS, ACT, T_TRAINED, ROW_OFFSET, SEED = 2, 8, 4, 2, 6, 3, 11
TD = OBS + ACT

SAMPLERS = ("ddpm4", "ddim3eta0", "ddim3eta0.5")
# (the last entry is the only one with both a condition beyond horizon step 0 and a projector: it holds their order)
ENTRIES = ("p_sample_loop", "policy", "cond0_shared", "cond0_rows_and_2", "guided", "projected", "guided_projected",
           "projected_cond0_rows_and_2")
CASES = ["-".join(c) for c in itertools.product(SAMPLERS, ("torch", "philox"), ("eager", "graph"),
                                                ("stack", "nostack"), ENTRIES)]


def _h(t) -> str:
    if t is None:
        return "-"
    return hashlib.sha1(np.ascontiguousarray(t.detach().numpy()).tobytes()).hexdigest()[:8]


def _ramp(shape, *ints) -> torch.Tensor:
    """A tensor of small exact values that differs for every different ``ints``."""
    k = sum(p * int(v) for p, v in zip((7, 11, 13, 17), ints))
    n = int(np.prod(shape))
    return (((torch.arange(n) * 5 + k) % 23 - 11).float() / 16).reshape(tuple(shape))


class RecordingEngine:
    """Stands where ``_engine.Engine`` stands for the loops: same method names, keywords and defaults."""

    def __init__(self, events):
        self.events = events
        self._pinned = {}

    def persistent(self, tag, shape):
        key = (tag, tuple(shape))
        if key not in self._pinned:
            self._pinned[key] = torch.zeros(tuple(shape))
        return self._pinned[key]

    def tag_of(self, t) -> str:
        if t is not None:
            for (tag, shape), buf in self._pinned.items():
                if t.data_ptr() == buf.data_ptr() and tuple(t.shape) == shape:
                    return tag
        return "-"

    def aliases_persistent(self, t) -> bool:
        lo, hi = t.data_ptr(), t.data_ptr() + 4 * t.numel()
        return any(lo < b.data_ptr() + 4 * b.numel() and b.data_ptr() < hi for b in self._pinned.values())

    def fill_normal(self, x, seed, row_offset=0, draw=0):
        self.events.append(f"fill s{seed} r{row_offset} d{draw}")
        x.copy_(_ramp(x.shape, seed, row_offset, draw))

    # ---------------------------------------------------------------- one step
    def _advance(self, x, ident, noise, seed, row_offset, draw, cond0, guide_grad, guide_weight):
        z = noise if noise is not None else _ramp(x.shape, seed, row_offset, draw)
        x.mul_(0.5).add_(z, alpha=0.25).add_(_ramp(x.shape, 0, 0, 0, ident), alpha=0.125)
        if guide_grad is not None:
            x.add_(guide_grad, alpha=0.0625 * guide_weight)
        if cond0 is not None:
            x[:, 0] = cond0.reshape(-1, x.shape[2])

    def _step(self, name, ident, x, noise, seed, row_offset, draw, cond0, guide_grad, guide_weight):
        self.events.append(f"{name} x{_h(x)} z{_h(noise)} s{seed} r{row_offset} d{draw} c{_h(cond0)} "
                           f"g{_h(guide_grad)} w{guide_weight:g}")
        self._advance(x, ident, noise, seed, row_offset, draw, cond0, guide_grad, guide_weight)

    def denoise_step(self, x, t, *, noise=None, seed=0, row_offset=0, draw=0, cond0=None, guide_grad=None,
                     guide_weight=0.0):
        self._step(f"step t{int(t)}", int(t), x, noise, seed, row_offset, draw, cond0, guide_grad, guide_weight)

    def sampler_step(self, x, coef, *, noise=None, seed=0, row_offset=0, draw=0, cond0=None, guide_grad=None,
                     guide_weight=0.0):
        row = hashlib.sha1(np.asarray(coef).tobytes()).hexdigest()[:8]
        self._step(f"sstep k{row}", int(row, 16) % 97, x, noise, seed, row_offset, draw, cond0, guide_grad,
                   guide_weight)

    # ---------------------------------------------------------------- the fused loop
    def _loop(self, name, idents, alphas, x, noise_stack, seed, row_offset, cond0, projection, use_graph):
        self.events.append(f"{name} x{_h(x)}@{self.tag_of(x)} z{_h(noise_stack)}@{self.tag_of(noise_stack)} "
                           f"c{_h(cond0)}@{self.tag_of(cond0)} s{seed} r{row_offset} p{int(projection is not None)} "
                           f"a{_alphas(alphas)} G{int(bool(use_graph))}")
        for j, ident in enumerate(idents):
            z = None if noise_stack is None else noise_stack[j]
            self._advance(x, ident, z, seed, row_offset, j + 1, cond0, None, 0.0)
            if projection is not None:
                projection.mix(x, alphas[j])

    def sample_loop(self, x, n_steps, *, noise_stack=None, seed=0, row_offset=0, cond0=None, projection=None,
                    proj_alphas=None, use_graph=False):
        ts = list(reversed(range(int(n_steps))))
        # dad_sample_loop reads entry t of the by-timestep table at the iteration that runs timestep t
        alphas = None if projection is None else [proj_alphas[t] for t in ts]
        self._loop(f"loop n{int(n_steps)}", ts, alphas, x, noise_stack, seed, row_offset, cond0, projection,
                   use_graph)

    def sampler_loop(self, x, steps, *, noise_stack=None, seed=0, row_offset=0, cond0=None, projection=None,
                     proj_alphas=None, use_graph=False):
        rows = [hashlib.sha1(np.asarray(s).tobytes()).hexdigest()[:8] for s in steps]
        if projection is not None:
            assert len(proj_alphas) == len(rows)
        self._loop("sloop k" + ",".join(rows), [int(r, 16) % 97 for r in rows],
                   None if projection is None else list(proj_alphas), x, noise_stack, seed, row_offset, cond0,
                   projection, use_graph)


def _alphas(alphas) -> str:
    return "-" if alphas is None else ",".join(f"{float(a):.6g}" for a in alphas)


class RecordingProjector:
    """Stands where ``ProjectionState`` stands: ``apply(x, alpha)`` in place."""

    def __init__(self, events):
        self.events = events

    def mix(self, x, alpha):
        x.mul_(1.0 - 0.25 * float(alpha)).add_(_ramp(x.shape, 1, 2, 3), alpha=0.125 * float(alpha))

    def apply(self, x, alpha):
        self.events.append(f"proj a{float(alpha):.6g} x{_h(x)}")
        self.mix(x, alpha)


def _guide(x, t):
    """Its gradient, x (t + 1) / 4, shows both the point and the timestep it was taken at."""
    return (x * x).sum(dim=(1, 2)) * 0.125 * (t.float() + 1.0)


def run_case(case: str) -> list:
    from dynamics_aware_diffusion_amd import DynamicsAwarePolicy, GaussianDiffusion, GuidedPolicy, TemporalUnet
    sampler, rng, graph, stack, entry = case.split("-")
    events = []
    diff = GaussianDiffusion(TemporalUnet(TD, dim=32, dim_mults=(1, 2)), HORIZON, OBS, ACT, n_timesteps=T_TRAINED)
    eng = RecordingEngine(events)
    diff._engine = lambda device: eng
    diff.sampler_rng, diff.seed, diff.use_graph = rng, SEED, graph == "graph"
    if stack == "nostack":
        diff.max_noise_stack_bytes = 0

    guided, projected = entry.startswith("guided"), "projected" in entry
    policy = None
    if projected:
        stats = types.SimpleNamespace(obs_mean=np.zeros(OBS, np.float32), obs_std=np.ones(OBS, np.float32),
                                      action_mean=np.zeros(ACT, np.float32), action_std=np.ones(ACT, np.float32))
        policy = DynamicsAwarePolicy(diff, projection_matrix=torch.eye(TD), normalizer=stats, state_dim=OBS,
                                     observation_dim=OBS, action_dim=ACT, horizon=HORIZON,
                                     projection_schedule="linear", projection_strength=0.75,
                                     project_during_sampling=True)
        policy._projector = RecordingProjector(events)
    elif entry != "p_sample_loop":
        policy = GuidedPolicy(diff, None)
    if guided:
        policy.guide_fn, policy.guide_weight = _guide, 0.5
    conditions = {"cond0_shared": {0: _ramp((1, TD), 5)},
                  "cond0_rows_and_2": {0: _ramp((B, TD), 6), 2: _ramp((B, TD), 7)}}.get(entry.replace("projected_", ""))

    # (the policy above read the trained length; the loops below run the lowered one, as evaluate.py lowers it)
    if sampler == "ddpm4":
        diff.n_timesteps = 4
    else:
        diff.set_sampler("ddim", steps=3, eta=float(sampler.split("eta")[1]))

    torch.manual_seed(1234)
    if policy is None:
        out = diff.p_sample_loop((B, HORIZON, TD), row_offset=ROW_OFFSET)
    else:
        out = policy.sample_loop(batch_size=B, conditions=conditions, row_offset=ROW_OFFSET)
    events.append(f"gen {_h(torch.randn(1))}")
    events.append(f"ret {_h(out)} alias{int(eng.aliases_persistent(out))}")
    return events
