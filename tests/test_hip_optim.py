"""GPU tests of the optimiser step (dad_optim_step, csrc/optim_step.hpp) and of what drives it (FusedAdam, Trainer,
TemporalUnet.mark_weights_changed): clip_grad_norm_ + torch.optim.Adam + the reference's EMA update
(utils/training.py:158-189) against a float64 restatement written here with numpy.

The gate, per tensor X (p, exp_avg, exp_avg_sq, ema) after n steps:

    max|X_hip - X_f64| <= 2 max|X_torch32 - X_f64| + n 2^-23 max|X_f64|

X_torch32 is clip_grad_norm_ + torch.optim.Adam + ``ema.mul_(d).add_(p, alpha=1 - d)`` in fp32 on the same inputs;
the floor is one fp32 rounding of the stored value per step on each side.  The gradient norm:
|norm_hip - norm_f64| <= 2 |norm_torch32 - norm_f64| + 2^-18 norm_f64 (up to 64 levels of fp32 adds).

Measured on an MI355X (worst over tensors and steps of the raw-list case, as a fraction of the gate): see DESIGN.md §3,
"Optimiser step".
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dynamics_aware_diffusion_amd import _engine
from dynamics_aware_diffusion_amd._engine import DadOptimArgs, DadOptimGroup, DadOptimTensor
from dynamics_aware_diffusion_amd.utils.training import FusedAdam, Trainer
from tests.test_hip_parity import TOL_STEP, dev  # noqa: F401  (the module-scoped device fixture)
from tests.test_optim_host import multi_chunk_size, plan_sizes

pytestmark = pytest.mark.gpu

BETAS, EPS, DECAY = (0.9, 0.999), 1e-8, 0.995
LRS = (1e-3, 3e-4, 2e-3, 5e-4)              # a different lr each step
NORMS = (3.0, 1.5, 0.5, 0.2)                # total gradient norm of each step: the first two clip at max_norm = 1
F23, F18 = 2.0 ** -23, 2.0 ** -18

CONFIGS = {                                  # weight_decay, decoupled, max_grad_norm
    "clip": (0.0, False, 1.0),
    "l2_decay": (0.01, False, 1.0),
    "decoupled_decay": (0.01, True, 1.0),
    "no_clip": (0.0, False, None),
}


# ----------------------------------------------------------------------------------- the three statements of a step
def f64_step(st, grads, lr, step, wd, decoupled, max_norm, decay=DECAY):
    """One step in float64, in place on st = {"p", "m", "v", "ema"} (lists of float64 arrays, ema entries may be
    None); grads entries may be None.  Returns the pre-clip total norm."""
    sq = sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grads if g is not None)
    norm = math.sqrt(sq)
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm else 1.0
    b1, b2 = BETAS
    for i, g in enumerate(grads):
        p = st["p"][i]
        if g is not None:
            g = coef * g.astype(np.float64)
            if wd:
                if decoupled:
                    p *= 1 - lr * wd
                else:
                    g = g + wd * p
            st["m"][i] += (g - st["m"][i]) * (1 - b1)
            st["v"][i] *= b2
            st["v"][i] += (1 - b2) * g * g
            p -= lr / (1 - b1 ** step) * st["m"][i] / (np.sqrt(st["v"][i]) / math.sqrt(1 - b2 ** step) + EPS)
        if st["ema"][i] is not None:
            st["ema"][i] *= decay
            st["ema"][i] += (1 - decay) * p
    return norm


class Torch32:
    """The parent's way in fp32 on the device: clip_grad_norm_, torch.optim.Adam, the reference's EMA expression."""

    def __init__(self, p, m, v, ema, has_grad, step0, wd, decoupled, max_norm, devc, decay=DECAY):
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(devc)     # noqa: E731
        self.p = [torch.nn.Parameter(t(a)) for a in p]
        self.ema = [t(a) for a in ema]
        self.trained = [q for q, h in zip(self.p, has_grad) if h]
        self.opt = torch.optim.Adam(self.trained or [torch.nn.Parameter(torch.zeros(1, device=devc))], lr=1.0, betas=BETAS,
                                    eps=EPS, weight_decay=wd, decoupled_weight_decay=decoupled)
        for q, a, b, h in zip(self.p, m, v, has_grad):
            if h:
                self.opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": t(a), "exp_avg_sq": t(b)}
        self.max_norm, self.decay = max_norm, decay

    def step(self, grads, lr):
        for q, g in zip(self.p, grads):
            q.grad = None if g is None else g.detach().clone()
        self.opt.param_groups[0]["lr"] = lr
        norm = None
        if self.max_norm:
            norm = float(torch.nn.utils.clip_grad_norm_(self.trained, self.max_norm))
        if self.trained:
            self.opt.step()
        with torch.no_grad():
            for e, q in zip(self.ema, self.p):
                if e is not None:
                    e.data.mul_(self.decay).add_(q.data, alpha=1 - self.decay)
        return norm

    def snapshot(self):
        zero = lambda q: np.zeros(tuple(q.shape), np.float32)                                       # noqa: E731
        n = lambda x: x.detach().cpu().numpy().copy()                                               # noqa: E731
        m = [n(self.opt.state[q]["exp_avg"]) if q in self.opt.state else zero(q) for q in self.p]
        v = [n(self.opt.state[q]["exp_avg_sq"]) if q in self.opt.state else zero(q) for q in self.p]
        return {"p": [n(q) for q in self.p], "m": m, "v": v, "ema": [None if e is None else n(e) for e in self.ema]}


class HipLists:
    """Raw tensor lists on the device behind one dad_optim; `unaligned` tensors are views 7 floats into flat buffers."""

    def __init__(self, p, ema, has_grad, unaligned, devc):
        self.lib = _engine.load_library()
        self.devc, self.has_grad, self.unaligned = devc, has_grad, unaligned
        self.p = [self.place(a, u) for a, u in zip(p, unaligned)]
        self.m = [self.place(np.zeros_like(a), u) if h else None for a, u, h in zip(p, unaligned, has_grad)]
        self.v = [self.place(np.zeros_like(a), u) if h else None for a, u, h in zip(p, unaligned, has_grad)]
        self.ema = [None if a is None else self.place(a, u) for a, u in zip(ema, unaligned)]
        for group, u in zip(zip(self.p, self.m, self.v, self.ema), unaligned):
            for x in group:
                assert x is None or (x.data_ptr() % 16 != 0) == u
        h = C.c_void_p()
        assert self.lib.dad_optim_create(C.byref(h)) == 0
        self.h = h
        self.norm = torch.full((), -1.0, device=devc)
        self.steps = 0

    def place(self, a, unaligned):
        if a is None:
            return None
        if not unaligned:
            return torch.from_numpy(np.ascontiguousarray(a)).to(self.devc)
        flat = torch.zeros(a.size + 9, device=self.devc)
        view = flat[7:7 + a.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return view

    def grads(self, arrays):
        """Fresh device allocations of a step's gradients (None where the tensor has none)."""
        return [None if a is None else self.place(a, u) for a, u in zip(arrays, self.unaligned)]

    def step(self, grads, lr, wd, decoupled, max_norm, decay=DECAY):
        self.steps += 1
        n = len(self.p)
        tab = (DadOptimTensor * n)()
        for i in range(n):
            r = tab[i]
            r.param, r.numel, r.group = self.p[i].data_ptr(), self.p[i].numel(), 0
            if grads[i] is not None:
                r.grad, r.exp_avg, r.exp_avg_sq = grads[i].data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr()
            if self.ema[i] is not None:
                r.ema = self.ema[i].data_ptr()
        group = (DadOptimGroup * 1)()
        FusedAdam._fill_group(group[0], dict(lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, decoupled_weight_decay=decoupled),
                              self.steps)
        a = DadOptimArgs()
        a.groups, a.n_groups, a.ema_decay = group, 1, decay
        a.max_grad_norm = max_norm or 0.0
        a.grad_norm_out = self.norm.data_ptr() if max_norm else None
        rc = self.lib.dad_optim_step(self.h, tab, n, C.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.lib.dad_last_error()

    def snapshot(self):
        n = lambda x: x.detach().cpu().numpy().copy()                                               # noqa: E731
        zero = lambda q: np.zeros(tuple(q.shape), np.float32)                                       # noqa: E731
        return {"p": [n(x) for x in self.p], "m": [zero(q) if x is None else n(x) for x, q in zip(self.m, self.p)],
                "v": [zero(q) if x is None else n(x) for x, q in zip(self.v, self.p)],
                "ema": [None if x is None else n(x) for x in self.ema]}

    def close(self):
        torch.cuda.synchronize()
        self.lib.dad_optim_destroy(self.h)


def check_gate(hip, t32, f64, n, label, worst):
    """The gate of the module docstring on every tensor of one snapshot; records the worst error / bound ratio."""
    for key in ("p", "m", "v", "ema"):
        for i, (a, b, c) in enumerate(zip(hip[key], t32[key], f64[key])):
            if c is None:
                assert a is None
                continue
            err = float(np.max(np.abs(a.astype(np.float64) - c)))
            ref = float(np.max(np.abs(b.astype(np.float64) - c)))
            bound = 2 * ref + n * F23 * float(np.max(np.abs(c)))
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
            if ratio > worst.get(key, (0.0,))[0]:
                worst[key] = (ratio, err, ref, bound, f"{label} tensor {i} ({a.size} elements)")
            assert err <= bound, f"{label} {key}[{i}] ({a.size} elements): |hip - f64| = {err:.3e} > {bound:.3e} (torch32 {ref:.3e})"


# ----------------------------------------------------------------------------------- (a) raw tensor lists
class Lists:
    """Inputs of the raw-list tests, made once: the plan-test sizes and the multi-chunk tensor with 16-byte aligned
    pointers, then the plan-test sizes and a 2-chunk tensor at pointers that are 4-byte aligned only."""

    def __init__(self):
        c = _engine.optim_plan([1])["chunk"]
        self.chunk = c
        self.sizes = plan_sizes() + [multi_chunk_size()] + plan_sizes() + [2 * c + 3]
        half = len(self.sizes) // 2
        self.big = half - 1
        self.unaligned = [i >= half for i in range(len(self.sizes))]
        self.no_grad = 4                          # the aligned 255-element tensor: EMA only
        self.no_ema = half + 6                    # the unaligned (chunk + 1)-element tensor
        self.five_unaligned = half + 3
        assert self.sizes[self.five_unaligned] == 5 and self.sizes[self.no_grad] == 255
        self.has_grad = [i != self.no_grad for i in range(len(self.sizes))]
        rng = np.random.default_rng(20240611)
        self.p = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in self.sizes]
        self.ema = [None if i == self.no_ema else (a + 0.01 * rng.standard_normal(a.size)).astype(np.float32)
                    for i, a in enumerate(self.p)]
        total = sum(n for n, h in zip(self.sizes, self.has_grad) if h)
        self.grads = [[(rng.standard_normal(n) * (norm / math.sqrt(total))).astype(np.float32) if h else None
                       for n, h in zip(self.sizes, self.has_grad)] for norm in NORMS]
        self.refs = {}

    def start64(self):
        return {"p": [a.astype(np.float64) for a in self.p], "m": [np.zeros(a.size) for a in self.p],
                "v": [np.zeros(a.size) for a in self.p], "ema": [None if a is None else a.astype(np.float64) for a in self.ema]}

    def reference(self, name, devc):
        """Per step (f64 snapshot, f64 norm, torch32 snapshot, torch32 norm) of a configuration; computed once."""
        if name not in self.refs:
            wd, decoupled, max_norm = CONFIGS[name]
            st = self.start64()
            zeros = [np.zeros_like(a) for a in self.p]
            t32 = Torch32(self.p, zeros, zeros, self.ema, self.has_grad, 0, wd, decoupled, max_norm, devc)
            out = []
            for k, lr in enumerate(LRS):
                n64 = f64_step(st, self.grads[k], lr, k + 1, wd, decoupled, max_norm)
                g = [None if a is None else torch.from_numpy(a).to(devc) for a in self.grads[k]]
                n32 = t32.step(g, lr)
                out.append(({key: [None if a is None else a.copy() for a in st[key]] for key in st}, n64, t32.snapshot(), n32))
            self.refs[name] = out
        return self.refs[name]

    def run_hip(self, name, devc, steps=len(LRS), sync=True, snapshots=True):
        wd, decoupled, max_norm = CONFIGS[name]
        hip = HipLists(self.p, self.ema, self.has_grad, self.unaligned, devc)
        out = []
        try:
            all_grads = [hip.grads(self.grads[k]) for k in range(steps)]      # different allocations, alive together
            if not sync:
                torch.cuda.synchronize()
            for k in range(steps):
                hip.step(all_grads[k], LRS[k], wd, decoupled, max_norm)
                if sync:
                    torch.cuda.synchronize()
                if snapshots:
                    out.append((hip.snapshot(), float(hip.norm)))
            if not snapshots:
                out.append((hip.snapshot(), float(hip.norm)))
        finally:
            hip.close()
        return out


@pytest.fixture(scope="module")
def lists():
    return Lists()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_raw_lists_against_float64(lists, dev, name):
    max_norm = CONFIGS[name][2]
    ref = lists.reference(name, dev)
    got = lists.run_hip(name, dev)
    worst = {}
    for k, ((hip, norm), (f64, n64, t32, n32)) in enumerate(zip(got, ref)):
        if max_norm:
            err, bound = abs(norm - n64), 2 * abs(n32 - n64) + F18 * n64
            print(f"{name} step {k + 1}: norm f64 {n64:.9g} |hip - f64| {err:.3e} |torch32 - f64| {abs(n32 - n64):.3e} bound {bound:.3e}")
            assert (n64 > max_norm) == (k < 2), "steps 1-2 clip, steps 3-4 do not"
            assert err <= bound
        check_gate(hip, t32, f64, k + 1, f"{name} step {k + 1}", worst)
    for key, (ratio, err, refe, bound, where) in sorted(worst.items()):
        print(f"{name} worst {key}: |hip - f64| {err:.3e} = {ratio:.3f} of the gate {bound:.3e} (torch32 {refe:.3e}) at {where}")
    # untouched: the moments of the EMA-only tensor do not exist, its parameter is unchanged, gradients are read only
    assert np.array_equal(got[-1][0]["p"][lists.no_grad], lists.p[lists.no_grad])
    assert got[-1][0]["ema"][lists.no_ema] is None


def test_second_run_is_bit_identical(lists, dev):
    a = lists.run_hip("clip", dev, snapshots=False)[0]
    b = lists.run_hip("clip", dev, snapshots=False)[0]
    assert a[1] == b[1]
    for key in ("p", "m", "v", "ema"):
        for x, y in zip(a[0][key], b[0][key]):
            assert (x is None and y is None) or x.tobytes() == y.tobytes(), key


# ----------------------------------------------------------------------------------- (b) no element is skipped by the norm
def _placements(lists):
    c, big, last = lists.chunk, lists.big, len(lists.sizes) - 1
    return {"first element of the first tensor": (0, 0),
            "last element of the last tensor": (last, lists.sizes[last] - 1),
            "element chunk - 1 of the multi-chunk tensor": (big, c - 1),
            "element chunk of the multi-chunk tensor": (big, c),
            "last element of the multi-chunk tensor": (big, lists.sizes[big] - 1),
            "last element of the unaligned 5-element tensor": (lists.five_unaligned, 4)}


@pytest.mark.parametrize("where", ["first element of the first tensor", "last element of the last tensor",
                                   "element chunk - 1 of the multi-chunk tensor", "element chunk of the multi-chunk tensor",
                                   "last element of the multi-chunk tensor", "last element of the unaligned 5-element tensor"])
def test_norm_sees_every_element(lists, dev, where):
    ti, ei = _placements(lists)[where]
    grads = [np.zeros(n, np.float32) if h else None for n, h in zip(lists.sizes, lists.has_grad)]
    grads[ti][ei] = 0.5
    lr, max_norm = 1e-3, 0.25
    hip = HipLists(lists.p, lists.ema, lists.has_grad, lists.unaligned, dev)
    try:
        hip.step(hip.grads(grads), lr, 0.0, False, max_norm)
        torch.cuda.synchronize()
        assert float(hip.norm) == 0.5
        got = hip.snapshot()
    finally:
        hip.close()
    # the first-step update of that element, within the gate (on a one-element "tensor": the element itself)
    one = lambda a: None if a is None else a[ei:ei + 1]                                              # noqa: E731
    st = {"p": [lists.p[ti][ei:ei + 1].astype(np.float64)], "m": [np.zeros(1)], "v": [np.zeros(1)],
          "ema": [None if lists.ema[ti] is None else lists.ema[ti][ei:ei + 1].astype(np.float64)]}
    assert f64_step(st, [np.float32([0.5])], lr, 1, 0.0, False, max_norm) == 0.5
    t32 = Torch32([one(lists.p[ti])], [np.zeros(1, np.float32)], [np.zeros(1, np.float32)], [one(lists.ema[ti])], [True], 0,
                  0.0, False, max_norm, dev)
    t32.step([torch.tensor([0.5], device=dev)], lr)
    worst = {}
    check_gate({k: [one(got[k][ti])] for k in got}, t32.snapshot(), st, 1, where, worst)
    assert abs(float(got["p"][ti][ei]) - float(lists.p[ti][ei])) > 0.5 * lr          # it did move, by about lr
    # ... and nothing else with a gradient of zero moved
    other = (ti + 1) % len(lists.sizes)
    if lists.has_grad[other]:
        assert np.array_equal(got["p"][other], lists.p[other])


# ----------------------------------------------------------------------------------- (c) re-upload
def test_moved_gradients_back_to_back(lists, dev):
    """Two steps whose gradient tensors are different allocations (the descriptor table is uploaded again for the second
    while the first may still run), issued without a synchronisation in between, against the same steps drained one by one."""
    queued = lists.run_hip("clip", dev, steps=2, sync=False, snapshots=False)[0]
    drained = lists.run_hip("clip", dev, steps=2, sync=True, snapshots=False)[0]
    assert queued[1] == drained[1]
    for key in ("p", "m", "v", "ema"):
        for x, y in zip(queued[0][key], drained[0][key]):
            assert (x is None and y is None) or x.tobytes() == y.tobytes(), key
    f64, _, t32, _ = lists.reference("clip", dev)[1]          # and they are the second step of the reference
    check_gate(queued[0], t32, f64, 2, "queued step 2", {})


# ----------------------------------------------------------------------------------- (d) through the net
def _tiny(devc, seed=5):
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    from dynamics_aware_diffusion_amd.utils import synth
    od, ad, dim, mults, T = synth.ARCHS["tiny"]
    state = synth.synth_unet_state(od + ad, dim, mults, seed=seed, affine_jitter=0.2)
    unet = TemporalUnet(od + ad, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return GaussianDiffusion(unet, 32, od, ad, n_timesteps=T).to(devc)


def _plan(diff, noise, devc):
    """A batch of plans under injected noise: x_T = noise[0], z of step j = noise[1 + j]."""
    eng = diff._engine(devc)
    x = noise[0].to(devc).clone()
    eng.sample_loop(x, int(diff.n_timesteps), noise_stack=noise[1:].to(devc).contiguous())
    torch.cuda.synchronize()
    return x.cpu().numpy()


class _F64Tail:
    """A copy of the net whose step is Trainer.train_step's with the tail in float64: the net runs in fp32 as it must,
    its parameters are the float64 masters rounded once per step; masters, moments and EMA stay in float64."""

    def __init__(self, diff, fused_objective, lr, clip, decay):
        diff.fused_objective = fused_objective
        self.diff, self.lr, self.clip, self.decay, self.steps = diff, lr, clip, decay, 0
        self.params = list(diff.parameters())
        self.p = [q.detach().double() for q in self.params]
        self.m = [torch.zeros_like(q) for q in self.p]
        self.v = [torch.zeros_like(q) for q in self.p]
        self.ema = [q.clone() for q in self.p]

    def train_step(self, x0):
        for q in self.params:
            q.grad = None
        with torch.enable_grad():
            self.diff.loss(x0).backward()
        self.steps += 1
        b1, b2 = BETAS
        grads = [q.grad.double() for q in self.params]
        norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
        coef = min(1.0, self.clip / (norm + 1e-6))
        with torch.no_grad():
            for q, p, m, v, e, g in zip(self.params, self.p, self.m, self.v, self.ema, grads):
                g = coef * g
                m += (g - m) * (1 - b1)
                v.mul_(b2).add_((1 - b2) * g * g)
                p -= self.lr / (1 - b1 ** self.steps) * m / (v.sqrt() / math.sqrt(1 - b2 ** self.steps) + EPS)
                e.mul_(self.decay).add_((1 - self.decay) * p)
                q.copy_(p.float())


@pytest.mark.parametrize("fused_objective", [False, True])
def test_trainer_fused_adam_against_the_reference_tail(dev, tmp_path, fused_objective):
    """Two copies of the tiny net take 3 Trainer.train_step's on the same batches and seeds: one with FusedAdam, one with
    torch.optim.Adam and the reference's tail (clip_grad_norm_, Adam, the .data EMA loop).  A third copy takes the same
    steps with the tail restated in float64 (``_F64Tail``): it is the X_f64 of the gate between the paths.

    What is asserted about the parameters.  (1) Every step of the FusedAdam copy, on ITS OWN inputs (its parameters,
    moments and EMA before the step and the gradient backward left in p.grad, which the step does not clip), meets the
    gate of the module docstring with n = 1 against the float64 restatement, X_torch32 being torch's tail on clones of
    the same inputs.  (2) The final parameters and EMA parameters, per tensor in max norm, meet gate (a) taken between
    the paths, each X the result of its own copy's three steps through the net:

        max|X_fused - X_f64| <= (2 K + 1) * 3 * 2^-23 max|X_f64|,   K = max over tensors of max|X_torch - X_f64| / (3 * 2^-23 max|X_f64|)

    i.e. the reference's own error enters in units of the floor and as its maximum over the tensors of the net, not
    tensor by tensor.  Why: the copies see the same gradients at step 1 only; from step 2 on their weights differ in
    the last bits, and the net and Adam's division by sqrt(v) amplify that, so the fp32 copies end several roundings
    apart (measured: FusedAdam against torch.optim.Adam up to 4.6 floors on the parameters, 2.4 on the EMA; either of
    them up to 33 floors from the float64 copy; DESIGN.md §3 "Optimiser step") and the floor alone cannot be met by
    any fp32 tail.  How far a
    rounding-level difference is amplified is a property of the net; the torch copy's distance from the float64 copy is
    one draw of it per tensor, and which tensor draws the largest value differs from path to path (tensor by tensor
    the torch copy itself sits anywhere between 0.11 and 33 floors), so the amplification is read off the reference as
    its worst tensor.  K comes from torch.optim.Adam's run alone; nothing in the bound depends on FusedAdam."""
    from dynamics_aware_diffusion_amd.utils import synth
    from dynamics_aware_diffusion_amd.utils.checkpoint import load_checkpoint
    lr, decay, clip, steps = 3e-3, 0.5, 1.0, 3
    copies = {}
    for which in ("fused", "torch"):
        diff = _tiny(dev)
        diff.fused_objective = fused_objective
        params = list(diff.parameters())
        opt = FusedAdam(params, lr=lr) if which == "fused" else torch.optim.Adam(params, lr=lr)
        copies[which] = Trainer(diff, opt, None, device=dev, log_dir=str(tmp_path / which), use_ema=True, ema_decay=decay,
                                gradient_clip=clip)
    fused, plain = copies["fused"], copies["torch"]
    exact = _F64Tail(_tiny(dev), fused_objective, lr, clip, decay)
    assert fused.fused and not plain.fused and fused.optimizer.max_grad_norm == clip
    td, T = fused.model.transition_dim, int(fused.model.n_timesteps)
    noise = torch.from_numpy(synth.normal_like(9, "optim.plan.noise", (T + 1, 4, 32, td)))
    before = {k: _plan(tr.ema_model, noise, dev) for k, tr in copies.items()}       # the EMA models' engines exist now
    assert np.array_equal(before["fused"], before["torch"])
    start = [p.detach().cpu().numpy().copy() for p in fused.model.parameters()]
    n = lambda ts: [None if t is None else t.detach().cpu().numpy().copy() for t in ts]              # noqa: E731
    worst = {}
    for k in range(steps):
        x0 = torch.from_numpy(synth.normal_like(9, f"optim.batch.{k}", (4, 32, td)))
        params, emas = list(fused.model.parameters()), list(fused.ema_model.parameters())
        state = fused.optimizer.state
        pre = {"p": n(params), "ema": n(emas),
               "m": n([state[p]["exp_avg"] if p in state else torch.zeros_like(p) for p in params]),
               "v": n([state[p]["exp_avg_sq"] if p in state else torch.zeros_like(p) for p in params])}
        losses = {}
        for which, tr in copies.items():
            torch.manual_seed(1000 + k)
            losses[which] = tr.train_step({"conditions": x0.clone()})["diffusion"]
        torch.manual_seed(1000 + k)
        exact.train_step(x0.clone().to(dev))
        print(f"step {k + 1}: loss fused {losses['fused']:.9g} torch {losses['torch']:.9g}")
        assert abs(losses["fused"] - losses["torch"]) <= 1e-5 * abs(losses["torch"])
        # (1) this step of the fused copy against float64 and torch32 on its own inputs
        grads = [p.grad for p in params]
        assert all(g is not None for g in grads)
        st = {key: [a.astype(np.float64).ravel() for a in pre[key]] for key in pre}
        norm64 = f64_step(st, [g.detach().cpu().numpy().ravel() for g in grads], lr, k + 1, 0.0, False, clip, decay)
        t32 = Torch32([a.ravel() for a in pre["p"]], [a.ravel() for a in pre["m"]], [a.ravel() for a in pre["v"]],
                      [a.ravel() for a in pre["ema"]], [True] * len(params), k, 0.0, False, clip, dev, decay)
        norm32 = t32.step([g.reshape(-1) for g in grads], lr)
        got = {"p": [a.ravel() for a in n(params)], "ema": [a.ravel() for a in n(emas)],
               "m": [a.ravel() for a in n([state[p]["exp_avg"] for p in params])],
               "v": [a.ravel() for a in n([state[p]["exp_avg_sq"] for p in params])]}
        check_gate(got, t32.snapshot(), st, 1, f"net step {k + 1}", worst)
        norm = float(fused.optimizer.last_grad_norm)
        print(f"step {k + 1}: grad norm f64 {norm64:.9g} |hip - f64| {abs(norm - norm64):.3e} |torch32 - f64| {abs(norm32 - norm64):.3e}")
        assert abs(norm - norm64) <= 2 * abs(norm32 - norm64) + F18 * norm64
        assert all(int(state[p]["step"]) == k + 1 for p in params)
    for key, (ratio, err, refe, bound, where) in sorted(worst.items()):
        print(f"net worst {key}: |hip - f64| {err:.3e} = {ratio:.3f} of the gate {bound:.3e} (torch32 {refe:.3e}) at {where}")
    # (2) gate (a) between the paths after 3 steps, per tensor in max norm
    for what, a, b, ref in (("parameters", fused.model, plain.model, exact.p), ("EMA parameters", fused.ema_model, plain.ema_model, exact.ema)):
        num = math.sqrt(sum(float(((x - y).double() ** 2).sum()) for x, y in zip(a.parameters(), b.parameters())))
        den = math.sqrt(sum(float(((y.detach().cpu().double() - torch.from_numpy(s0).double()) ** 2).sum())
                            for y, s0 in zip(b.parameters(), start)))
        floors = max(float((x - y).abs().max()) / (steps * F23 * float(y.abs().max())) for x, y in zip(a.parameters(), b.parameters()))
        print(f"{what}: |fused - torch|_2 = {num:.3e}, |torch - start|_2 = {den:.3e}, ratio {num / den:.3e}; "
              f"worst tensor max|fused - torch| = {floors:.2f} x (n 2^-23 max|X|)")
        rows = []
        for i, (x, y, z) in enumerate(zip(a.parameters(), b.parameters(), ref)):
            floor = steps * F23 * float(z.abs().max())
            rows.append((float((x.detach().double() - z).abs().max()) / floor, float((y.detach().double() - z).abs().max()) / floor, i, x.numel()))
        K = max(r[1] for r in rows)
        worst_row = max(rows)
        print(f"{what} between the paths, in floors (3 * 2^-23 max|X_f64|): torch copy K = {K:.2f} (smallest {min(r[1] for r in rows):.2f}), "
              f"fused copy worst {worst_row[0]:.2f} at tensor {worst_row[2]} ({worst_row[3]} elements, torch copy there {worst_row[1]:.2f}), "
              f"gate {2 * K + 1:.2f}")
        for fused_floors, torch_floors, i, numel in rows:
            assert fused_floors <= 2 * K + 1, (f"{what} tensor {i} ({numel} elements): |fused - f64| = {fused_floors:.2f} floors > "
                                               f"{2 * K + 1:.2f} (torch copy: {torch_floors:.2f} here, {K:.2f} at its worst tensor)")
    # sampling afterwards: the EMA model of each trainer samples with its NEW weights (a stale engine would return `before`)
    for which, tr in copies.items():
        path = tr.save_checkpoint(0)
        fresh = load_checkpoint(path, device=dev, use_ema=True)
        want = _plan(fresh, noise, dev)
        got = _plan(tr.ema_model, noise, dev)
        moved = float(np.max(np.abs(want - before[which])))
        print(f"{which}: max|ema plan - fresh plan| = {np.max(np.abs(got - want)):.3e}, moved since before training {moved:.3e}")
        assert np.max(np.abs(got - want)) <= TOL_STEP
        assert moved > 1e-3
        # ... and so does the trained model itself
        assert np.max(np.abs(_plan(tr.model, noise, dev) - _plan(load_checkpoint(path, device=dev), noise, dev))) <= TOL_STEP
        tr.log_file.close()
    # the optimiser state is torch.optim.Adam's
    params = list(fused.model.parameters())
    adam = torch.optim.Adam(params, lr=lr)
    adam.load_state_dict(fused.optimizer.state_dict())
    again = FusedAdam(params, lr=lr)
    again.load_state_dict(adam.state_dict())
    for p in params:
        assert float(adam.state[p]["step"]) == steps == float(again.state[p]["step"])
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(adam.state[p][key], fused.optimizer.state[p][key])
            assert torch.equal(again.state[p][key], fused.optimizer.state[p][key])
    assert again.state_dict()["param_groups"] == adam.state_dict()["param_groups"]


# ----------------------------------------------------------------------------------- (e) mark_weights_changed
def test_mark_weights_changed_after_a_data_update(dev):
    from dynamics_aware_diffusion_amd.utils import synth
    diff, other = _tiny(dev, seed=5), _tiny(dev, seed=6)
    td, T = diff.transition_dim, int(diff.n_timesteps)
    noise = torch.from_numpy(synth.normal_like(9, "optim.mark.noise", (T + 1, 4, 32, td)))
    before = _plan(diff, noise, dev)                            # the engine exists
    decay = 0.5
    for ema_param, param in zip(diff.parameters(), other.parameters()):       # the reference's update, word for word
        ema_param.data.mul_(decay).add_(param.data, alpha=1 - decay)
    diff.model.mark_weights_changed()
    got = _plan(diff, noise, dev)
    fresh = _tiny(dev, seed=7)
    fresh.load_state_dict(diff.state_dict())
    want = _plan(fresh, noise, dev)
    assert np.max(np.abs(got - want)) <= TOL_STEP
    assert np.max(np.abs(got - before)) > 1e-3


# ----------------------------------------------------------------------------------- edges of the step
def test_step_without_any_gradient_reports_a_zero_norm(dev):
    """EMA-only tensors: clip_grad_norm_ of no gradients is 0; the EMA copies still move."""
    p = [np.full(5, 2.0, np.float32), np.full(300, -1.0, np.float32)]
    ema = [np.zeros(5, np.float32), np.zeros(300, np.float32)]
    hip = HipLists(p, ema, [False, False], [False, True], dev)
    try:
        assert float(hip.norm) == -1.0
        hip.step([None, None], 1e-3, 0.0, False, 1.0, decay=0.75)
        torch.cuda.synchronize()
        assert float(hip.norm) == 0.0
        got = hip.snapshot()
    finally:
        hip.close()
    assert np.array_equal(got["ema"][0], np.full(5, 0.5, np.float32)) and np.array_equal(got["ema"][1], np.full(300, -0.25, np.float32))
    assert np.array_equal(got["p"][0], p[0]) and np.array_equal(got["p"][1], p[1])


def test_refused_step_leaves_the_step_counts_alone(dev):
    """Nine param groups are nine ABI groups: refused before the library is called; state['step'] and its host copy agree."""
    params = [torch.nn.Parameter(torch.ones(4, device=dev)) for _ in range(9)]
    opt = FusedAdam([{"params": [q], "lr": 1e-3 * (i + 1)} for i, q in enumerate(params)])
    for q in params:
        q.grad = torch.ones_like(q)
    with pytest.raises(ValueError, match="more than 8"):
        opt.step()
    assert all(float(opt.state[q]["step"]) == 0.0 for q in params) and not opt._steps
    assert all(torch.equal(q.detach(), torch.ones_like(q)) for q in params)
    opt.param_groups[8]["params"][0].grad = None              # eight groups with a gradient: the step goes through
    opt.step()
    torch.cuda.synchronize()
    assert [float(opt.state[q]["step"]) for q in params] == [1.0] * 8 + [0.0]
    assert all(float(q.detach().max()) < 1.0 for q in params[:8]) and torch.equal(params[8].detach(), torch.ones(4, device=dev))
