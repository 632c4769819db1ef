"""Training utilities: the mirror of the reference's ``m_diffuser/utils/training.py`` public names (``EMA``,
``Trainer``, ``CosineAnnealingWarmup``, ``count_parameters``) plus ``FusedAdam``, which runs everything the
reference's ``Trainer.train_step`` does after ``loss.backward()`` (utils/training.py:158-189: ``clip_grad_norm_``,
``torch.optim.Adam.step()`` and the ``update_ema`` loop) as one library call of at most two launches
(``dad_optim_step``, csrc/optim_step.hpp).

One difference from ``clip_grad_norm_``: ``FusedAdam`` applies the clip coefficient inside the update and leaves
``p.grad`` as ``backward`` wrote it, unclipped.

The engine of a ``TemporalUnet`` notices changed weights through ``(data_ptr, _version)`` of its parameters.
``FusedAdam`` writes parameters from a kernel and the reference's EMA loop writes through ``.data``; neither bumps
a version counter by itself, so both end by bumping them (``torch.autograd.graph.increment_version``), and the next
call of each model refreshes its engine.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import os
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn
from torch.autograd.graph import increment_version
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LRScheduler

from .. import _engine
from .._engine import DadOptimArgs, DadOptimGroup, DadOptimTensor, OPTIM_MAX_GROUPS


class FusedAdam(Optimizer):
    """``torch.optim.Adam`` (and AdamW with ``decoupled_weight_decay``) whose step also clips the global gradient
    norm (``max_grad_norm``, the arithmetic of ``clip_grad_norm_``) and updates EMA copies of the parameters
    (``ema_params``, ``ema_decay``: the reference's ``update_ema``), on the HIP library.

    The state per parameter is ``step`` / ``exp_avg`` / ``exp_avg_sq`` exactly as ``torch.optim.Adam`` keeps it, and
    the param groups carry Adam's keys: a ``state_dict()`` loads into ``torch.optim.Adam`` and back.  ``lr`` is read
    from ``param_groups`` at every step, so any LR scheduler drives it.  ``p.grad`` keeps the unclipped gradient.
    ``last_grad_norm`` is the pre-clip total norm of the last step as a device tensor (never synchronised); it is
    ``None`` without clipping.  fp32 CUDA parameters on one device only; there is no fallback.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 decoupled_weight_decay: bool = False, max_grad_norm: Optional[float] = None,
                 ema_params: Optional[Iterable[torch.Tensor]] = None, ema_decay: float = 0.995, *,
                 amsgrad: bool = False, maximize: bool = False):
        if amsgrad:
            raise ValueError("FusedAdam does not implement amsgrad")
        if maximize:
            raise ValueError("FusedAdam does not implement maximize")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # (the keys of torch.optim.Adam's groups, so that the two state dicts are interchangeable)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.ema_decay = float(ema_decay)
        self._reset_native()
        if ema_params is not None:
            self.set_ema([p for g in self.param_groups for p in g["params"]], ema_params, ema_decay)

    # ------------------------------------------------------------------ configuration
    def set_ema(self, params: Iterable[torch.Tensor], ema_params: Iterable[torch.Tensor], decay: float) -> None:
        """Pair parameters with their EMA copies (``zip(model.parameters(), ema_model.parameters())``).  A parameter
        that is in no param group, or has no gradient at a step, still has its EMA updated, as ``update_ema`` does."""
        params, ema_params = list(params), list(ema_params)
        if len(params) != len(ema_params):
            raise ValueError(f"{len(params)} parameters but {len(ema_params)} EMA tensors")
        for p, e in zip(params, ema_params):
            self._check_tensor(p, "parameter")
            self._check_tensor(e, "EMA tensor")
            if e.shape != p.shape or e.device != p.device:
                raise ValueError(f"EMA tensor {tuple(e.shape)} on {e.device} does not match its parameter "
                                 f"{tuple(p.shape)} on {p.device}")
        self._ema_pairs = list(zip(params, ema_params))
        self._ema = {id(p): e for p, e in self._ema_pairs}
        self.ema_decay = float(decay)
        self._layout = None

    @staticmethod
    def _check_tensor(t: torch.Tensor, what: str) -> None:
        if not t.is_cuda:
            raise ValueError(f"FusedAdam: {what} on {t.device}: the step runs on a ROCm device only")
        if t.dtype != torch.float32:
            raise ValueError(f"FusedAdam: {what} is {t.dtype}, not float32")
        if t.is_sparse:
            raise ValueError(f"FusedAdam: sparse {what}")
        if not t.is_contiguous():
            raise ValueError(f"FusedAdam: {what} is not contiguous")

    def _reset_native(self) -> None:
        self.last_grad_norm: Optional[torch.Tensor] = None
        self._ema: Dict[int, torch.Tensor] = {}           # id(param) -> its EMA tensor
        self._ema_pairs: List = []                        # (param, ema) in the order given
        self._lib = None
        self._handle = None
        self._table = None                                # ctypes array of DadOptimTensor, kept between steps
        self._rows: List = []                             # per row: [param, has a gradient, param group]
        self._touched: List = []                          # tensors a step writes
        self._layout = None                               # what the rows were built for
        self._steps: Dict[int, int] = {}                  # id(param) -> step count (host copy of state['step'])
        self._groups = (DadOptimGroup * OPTIM_MAX_GROUPS)()
        self._args = DadOptimArgs()

    def __setstate__(self, state):
        """Unpickling restores what torch.optim.Optimizer pickles (defaults, state, param groups); the clip threshold
        and the EMA pairs are set again by the caller."""
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("ema_decay", 0.995)
        if "_handle" not in self.__dict__:          # (load_state_dict passes through here too: it keeps the handle)
            self._reset_native()
        self._steps = {}
        self._layout = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdam does not implement amsgrad / maximize")
        self._steps = {}
        self._layout = None

    def __del__(self):
        if getattr(self, "_handle", None) is not None and self._lib is not None:
            self._lib.dad_optim_destroy(self._handle)
            self._handle = None

    # ------------------------------------------------------------------ the step
    def _init_state(self, p: torch.Tensor) -> dict:
        st = self.state[p]
        if len(st) == 0:
            self._check_tensor(p, "parameter")
            st["step"] = torch.tensor(0.0, dtype=torch.float32)          # on the host, as torch.optim.Adam keeps it
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _grad(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        g = p.grad
        if g is None:
            return None
        if g.is_sparse:
            raise ValueError("FusedAdam does not support sparse gradients")
        if g.dtype != torch.float32 or g.device != p.device:
            raise ValueError(f"FusedAdam: gradient is {g.dtype} on {g.device}, its parameter float32 on {p.device}")
        if not g.is_contiguous():
            g = g.contiguous()
            p.grad = g
        return g

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # rows of the table: every parameter of the groups that has a gradient (or an EMA copy), then the EMA pairs
        # that are in no group.  Built once; afterwards only the gradient pointers are looked at.
        have = tuple(p.grad is not None for g in self.param_groups for p in g["params"])
        layout = (have, tuple(len(g["params"]) for g in self.param_groups), len(self._ema_pairs))
        if layout != self._layout:
            self._build_rows()
            self._layout = layout
        rows, table = self._rows, self._table
        if not rows:
            return loss
        # the ABI groups: one per (param group, step count)
        keys: Dict = {}
        stepped, new_steps = [], {}                 # committed once the library has taken the step
        device = rows[0][0].device
        for i, row in enumerate(rows):
            p, gi = row[0], row[2]
            if p.device != device:
                raise ValueError(f"FusedAdam: parameters on {device} and {p.device}")
            if row[1]:                             # has a gradient: an Adam update
                g = self._grad(p)
                st = self.state[p]
                step = self._steps.get(id(p))
                if step is None:
                    step = int(st["step"])
                step += 1
                new_steps[id(p)] = step
                stepped.append(st["step"])
                table[i].grad = g.data_ptr()
                if table[i].param != p.data_ptr() or table[i].exp_avg != st["exp_avg"].data_ptr():
                    self._check_tensor(p, "parameter")
                    self._check_tensor(st["exp_avg"], "exp_avg")
                    self._check_tensor(st["exp_avg_sq"], "exp_avg_sq")
                    table[i].param = p.data_ptr()
                    table[i].exp_avg = st["exp_avg"].data_ptr()
                    table[i].exp_avg_sq = st["exp_avg_sq"].data_ptr()
                key = (gi, step)
            else:
                table[i].param = p.data_ptr()
                key = (gi, 0)
            slot = keys.get(key)
            if slot is None:
                slot = keys[key] = len(keys)
                if slot >= OPTIM_MAX_GROUPS:
                    raise ValueError(f"FusedAdam: more than {OPTIM_MAX_GROUPS} distinct (param group, step count) pairs "
                                     "in one step")
                self._fill_group(self._groups[slot], self.param_groups[max(gi, 0)], key[1])
            table[i].group = slot
            e = self._ema.get(id(p))
            if e is not None:
                table[i].ema = e.data_ptr()
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip and (self.last_grad_norm is None or self.last_grad_norm.device != device):
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=device)
        if not clip:
            self.last_grad_norm = None
        a = self._args
        a.groups = self._groups
        a.n_groups = len(keys)
        a.max_grad_norm = float(self.max_grad_norm) if clip else 0.0
        a.ema_decay = self.ema_decay
        a.grad_norm_out = self.last_grad_norm.data_ptr() if clip else None
        if self._handle is None:
            self._lib = _engine.load_library()
            h = C.c_void_p()
            _engine._check(self._lib, self._lib.dad_optim_create(C.byref(h)))
            self._handle = h
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _engine._check(self._lib, self._lib.dad_optim_step(self._handle, table, len(rows), C.byref(a), stream))
        # the step is enqueued: only now do the step counts advance (a refused step leaves state['step'] and its host
        # copy as they were)
        self._steps.update(new_steps)
        if stepped:
            torch._foreach_add_(stepped, 1)
        # the kernel wrote the tensors behind autograd's back: bump their versions, so that an engine built from them
        # (TemporalUnet.engine checks (data_ptr, _version)) refreshes itself at its next call
        increment_version(self._touched)
        return loss

    def _build_rows(self) -> None:
        rows = []
        in_groups = set()
        for gi, g in enumerate(self.param_groups):
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdam does not implement amsgrad / maximize")
            for p in g["params"]:
                in_groups.add(id(p))
                if p.grad is not None:
                    self._init_state(p)
                    rows.append([p, True, gi])
                elif id(p) in self._ema:
                    self._check_tensor(p, "parameter")
                    rows.append([p, False, gi])
        for p, _ in self._ema_pairs:
            if id(p) not in in_groups:
                rows.append([p, False, -1])
        self._rows = rows
        self._table = (DadOptimTensor * max(len(rows), 1))()
        for i, (p, _, _) in enumerate(rows):
            self._table[i].numel = p.numel()
        # what the kernel writes: the parameters that take an Adam update and every EMA copy (the parameter of an
        # EMA-only row is only read)
        self._touched = [r[0] for r in rows if r[1]] + [self._ema[id(r[0])] for r in rows if id(r[0]) in self._ema]

    @staticmethod
    def _fill_group(out: DadOptimGroup, g: dict, step: int) -> None:
        """The scalars of one (param group, step count), computed in double as torch.optim.Adam computes them."""
        lr = float(g["lr"])
        beta1, beta2 = (float(b) for b in g["betas"])
        out.lr, out.beta1, out.beta2, out.eps = lr, beta1, beta2, float(g["eps"])
        out.weight_decay = float(g["weight_decay"])
        out.decoupled = int(bool(g.get("decoupled_weight_decay", False)))
        out.one_minus_beta1, out.one_minus_beta2 = 1 - beta1, 1 - beta2
        if step > 0:
            out.step_size = lr / (1 - beta1 ** step)
            out.bc2_sqrt = math.sqrt(1 - beta2 ** step)
        else:                                      # EMA-only rows read no Adam scalar
            out.step_size, out.bc2_sqrt = 0.0, 1.0


class EMA:
    """Shadow copies of a model's trainable parameters, by name (the reference's ``EMA``, utils/training.py:18-62):
    ``update()`` moves every shadow towards its parameter, ``shadow = decay shadow + (1 - decay) p``;
    ``apply_shadow()`` puts the shadows into the model for evaluation and ``restore()`` puts the weights back."""

    def __init__(self, model: nn.Module, decay: float = 0.995):
        self.model = model
        self.decay = decay
        self.shadow: Dict[str, torch.Tensor] = {n: p.detach().clone() for n, p in self._tracked()}
        self.backup: Dict[str, torch.Tensor] = {}

    def _tracked(self):
        return [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]

    @torch.no_grad()
    def update(self) -> None:
        tracked = self._tracked()
        missing = [n for n, _ in tracked if n not in self.shadow]
        assert not missing, f"parameters without a shadow: {missing[:3]}"
        # new tensors rather than in-place: a shadow that apply_shadow() handed to the model is not changed under it
        for n, p in tracked:
            self.shadow[n] = torch.add(self.decay * self.shadow[n], p.detach(), alpha=1.0 - self.decay)

    def apply_shadow(self) -> None:
        for n, p in self._tracked():
            assert n in self.shadow, n
            self.backup[n], p.data = p.data, self.shadow[n]      # (another data_ptr: the model's engine rebuilds)

    def restore(self) -> None:
        for n, p in self._tracked():
            assert n in self.backup, n
            p.data = self.backup.pop(n)
        self.backup = {}


class Trainer:
    """The reference's training loop (utils/training.py:65-279), same constructor and methods.

    With a ``FusedAdam`` the trainer hands it ``gradient_clip`` and the EMA model's parameters: ``optimizer.step()``
    is then the whole tail of the step, and torch's ``clip_grad_norm_`` and the EMA loop are skipped.  With any other
    optimiser it does what the reference does; ``update_ema`` ends by bumping the EMA parameters' version counters,
    so an EMA model that has sampled before samples with its new weights."""

    def __init__(self, model, optimizer, train_loader, scheduler=None, device="cuda", log_dir="./logs",
                 save_freq=10000, eval_freq=5000, use_ema=True, ema_decay=0.995, gradient_clip=1.0,
                 loss_fn=None, loss_names=None):
        self.model = model
        self.optimizer = optimizer
        self.train_loader = train_loader
        self.scheduler = scheduler
        self.device = device
        self.log_dir = log_dir
        self.save_freq = save_freq
        self.eval_freq = eval_freq
        self.use_ema = use_ema
        self.gradient_clip = gradient_clip
        self.loss_fn = loss_fn
        self.loss_names = loss_names if loss_names else ["loss"]
        self.model.to(device)
        if use_ema:
            self.ema_model = copy.deepcopy(model)
            self.ema_decay = ema_decay
        else:
            self.ema_model = None
        self.fused = isinstance(optimizer, FusedAdam)
        if self.fused:
            optimizer.max_grad_norm = gradient_clip if gradient_clip and gradient_clip > 0 else None
            if self.ema_model is not None:
                optimizer.set_ema(self.model.parameters(), self.ema_model.parameters(), ema_decay)
        self.global_step = 0
        os.makedirs(log_dir, exist_ok=True)
        self.log_file = open(os.path.join(log_dir, "training.log"), "a")

    def compute_loss(self, batch):
        """(loss, dict of its components as floats for logging)"""
        if self.loss_fn is None:
            loss = self.model.loss(batch["conditions"])
            return loss, {"diffusion": loss.item()}
        out = self.loss_fn(batch)
        if isinstance(out, tuple):                  # a composed loss: (total, components)
            return out
        return out, {self.loss_names[0]: out.item()}

    def train_step(self, batch):
        for key in batch:
            if isinstance(batch[key], torch.Tensor):
                batch[key] = batch[key].to(self.device)
        with torch.enable_grad():
            loss, loss_dict = self.compute_loss(batch)
            self.optimizer.zero_grad()
            loss.backward()
        if self.fused:
            self.optimizer.step()                   # clip + Adam + EMA
            if self.scheduler is not None:
                self.scheduler.step()
        else:
            if self.gradient_clip > 0:
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.gradient_clip)
            self.optimizer.step()
            if self.scheduler is not None:
                self.scheduler.step()
            if self.ema_model is not None:
                self.update_ema()
        self.global_step += 1
        return loss_dict

    def update_ema(self) -> None:
        """ema = decay ema + (1 - decay) p over every parameter (utils/training.py:180-189)."""
        with torch.no_grad():
            ema_params = list(self.ema_model.parameters())
            for ema_param, param in zip(ema_params, self.model.parameters()):
                ema_param.data.mul_(self.ema_decay).add_(param.data, alpha=1 - self.ema_decay)
            increment_version(ema_params)           # (.data updates bump no version: the EMA model's engine must see them)

    def save_checkpoint(self, epoch, is_best=False):
        checkpoint = {
            "epoch": epoch,
            "global_step": self.global_step,
            "model_state_dict": self.model.state_dict(),
            "optimizer_state_dict": self.optimizer.state_dict(),
            "config": {
                "horizon": self.model.horizon,
                "observation_dim": self.model.observation_dim,
                "action_dim": self.model.action_dim,
                "n_timesteps": self.model.n_timesteps,
                "beta_schedule": self.model.beta_schedule,
            },
        }
        if self.ema_model is not None:
            checkpoint["ema_state_dict"] = self.ema_model.state_dict()
        if self.scheduler is not None:
            checkpoint["scheduler_state_dict"] = self.scheduler.state_dict()
        save_path = os.path.join(self.log_dir, f"checkpoint_step_{self.global_step}.pt")
        torch.save(checkpoint, save_path)
        if is_best:
            torch.save(checkpoint, os.path.join(self.log_dir, "checkpoint_best.pt"))
        return save_path

    def train(self, n_epochs, start_epoch=0):
        """``n_epochs`` passes over ``train_loader``: a checkpoint every ``save_freq`` steps and one at the end, a
        summary per epoch on stdout and in ``training.log``, a tqdm bar where tqdm is installed."""
        try:
            from tqdm import tqdm
        except ImportError:
            tqdm = None
        self.model.train()
        last = start_epoch + n_epochs
        for epoch in range(start_epoch, last):
            bar = None if tqdm is None else tqdm(self.train_loader, desc=f"Epoch {epoch + 1}/{last}")
            self._report(epoch, self._run_epoch(epoch, bar))
        print(f"\nFinal checkpoint saved: {self.save_checkpoint(last - 1)}")
        self.log_file.close()

    def _run_epoch(self, epoch, bar):
        """One pass over the loader; returns name -> the values ``train_step`` reported under it."""
        seen = {name: [] for name in self.loss_names}
        for batch in (self.train_loader if bar is None else bar):
            reported = self.train_step(batch)
            for name, values in seen.items():
                if name in reported:
                    values.append(reported[name])
            if bar is not None:
                bar.set_postfix({**{name: f"{reported.get(name, 0):.4f}" for name in self.loss_names},
                                 "lr": f"{self.optimizer.param_groups[0]['lr']:.2e}"})
            if self.global_step % self.save_freq == 0:
                print(f"\nSaved checkpoint: {self.save_checkpoint(epoch)}")
        return seen

    def _report(self, epoch, seen) -> None:
        print(f"\nEpoch {epoch + 1} Summary:")
        for name, values in seen.items():
            if values:
                mean = math.fsum(values) / len(values)
                print(f"  {name.capitalize()} loss: {mean:.4f}")
                self.log_file.write(f"Epoch {epoch + 1}, {name}: {mean:.4f}\n")
        self.log_file.flush()


class CosineAnnealingWarmup(LRScheduler):
    """Linear warm-up over ``warmup_steps``, then a cosine from the base rate down to ``min_lr`` at ``total_steps``
    (utils/training.py:284-320)."""

    def __init__(self, optimizer: Optimizer, warmup_steps: int, total_steps: int, min_lr: float = 0.0,
                 last_epoch: int = -1):
        self.warmup_steps = warmup_steps
        self.total_steps = total_steps
        self.min_lr = min_lr
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        step = self.last_epoch
        if step < self.warmup_steps:
            scale = step / self.warmup_steps
        else:
            progress = (step - self.warmup_steps) / (self.total_steps - self.warmup_steps)
            scale = 0.5 * (1.0 + math.cos(math.pi * progress))
        return [base * scale + self.min_lr * (1 - scale) for base in self.base_lrs]


def count_parameters(model: nn.Module) -> int:
    """Trainable parameters of a model."""
    return sum(p.numel() for p in model.parameters() if p.requires_grad)
