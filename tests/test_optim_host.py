"""CPU tests (`-m "not gpu"`) of the optimiser step's host side: the work split dad_optim_step replays
(dad_debug_optim_plan), its argument checks (made before any device call, so they run without a GPU), the refusals
of FusedAdam's constructor and the CosineAnnealingWarmup schedule against its closed form."""
import ctypes as C
import math
import os

import pytest
import torch

from dynamics_aware_diffusion_amd import _engine
from dynamics_aware_diffusion_amd._engine import DadOptimArgs, DadOptimGroup, DadOptimTensor

DAD_E_INVALID = -1


def _chunk() -> int:
    return _engine.optim_plan([1])["chunk"]


def plan_sizes():
    """The sizes every optimiser test uses: around the 4-element vector width, below / at / just past one chunk, a few
    chunks with a ragged end."""
    c = _chunk()
    return [1, 3, 4, 5, 255, c, c + 1, 3 * c + 5]


def multi_chunk_size() -> int:
    """The smallest tensor (plus a ragged end) whose chunks outnumber the largest grid: some block owns two."""
    head = _engine.optim_plan([1])
    c = head["chunk"]
    n = c
    while True:                     # grid grows with the chunks until it is capped
        p = _engine.optim_plan([n * c + 17])
        if p["chunks"] > p["grid"]:
            return n * c + 17
        n *= 2


def _check_plan(numel):
    p = _engine.optim_plan(numel)
    c = p["chunk"]
    assert c > 0 and c % 4 == 0
    assert p["partials"] == p["grid"] and 0 < p["grid"] <= 2048
    assert len(p["records"]) == p["chunks"]
    covered = [[] for _ in numel]
    last_of_block = {}
    for i, r in enumerate(p["records"]):
        assert 0 <= r["tensor"] < len(numel) and 0 <= r["block"] < p["grid"]
        assert r["first"] % 4 == 0 and 0 < r["count"] <= c
        assert r["first"] + r["count"] <= numel[r["tensor"]]
        covered[r["tensor"]].append((r["first"], r["count"]))
        # a block's chunks in ascending order: by (tensor, first element), which is the record order
        key = (r["tensor"], r["first"])
        assert r["block"] not in last_of_block or last_of_block[r["block"]] < key
        last_of_block[r["block"]] = key
    assert sorted(last_of_block) == list(range(p["grid"])), "a block without a chunk"
    for t, spans in enumerate(covered):           # every element in exactly one chunk
        at = 0
        for first, count in sorted(spans):
            assert first == at
            at += count
        assert at == numel[t]
    return p


def test_plan_covers_every_element_once():
    p = _check_plan(plan_sizes())
    assert p["chunks"] == 12 and p["grid"] == 12            # 6 one-chunk tensors, then 2 and 4 chunks


def test_plan_of_a_tensor_whose_blocks_walk_several_chunks():
    n = multi_chunk_size()
    p = _check_plan([5, n, 3])
    per_block = {}
    for r in p["records"]:
        per_block[r["block"]] = per_block.get(r["block"], 0) + 1
    assert max(per_block.values()) > 1 and p["grid"] <= 2048 < p["chunks"]


def test_plan_refuses_bad_sizes():
    lib = _engine.load_library()
    needed = C.c_int32()
    for sizes in ([0], [4, -1]):
        arr = (C.c_int64 * len(sizes))(*sizes)
        assert lib.dad_debug_optim_plan(arr, len(sizes), None, 0, C.byref(needed)) == DAD_E_INVALID
        assert lib.dad_last_error()
    assert lib.dad_debug_optim_plan(None, 1, None, 0, C.byref(needed)) == DAD_E_INVALID
    arr = (C.c_int64 * 1)(4)
    assert lib.dad_debug_optim_plan(arr, 0, None, 0, C.byref(needed)) == DAD_E_INVALID


def _tensor(**kw):
    """A descriptor of made-up (never dereferenced) device addresses; keywords override fields."""
    t = DadOptimTensor()
    t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.ema, t.numel, t.group = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 16, 0
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def _args(n_groups=1, groups=True):
    g = (DadOptimGroup * 9)()
    a = DadOptimArgs()
    a.groups = g if groups else None
    a.n_groups, a.max_grad_norm, a.ema_decay, a.grad_norm_out = n_groups, 1.0, 0.995, None
    return a, g


BAD_STEPS = {
    "null optimiser": dict(handle=False),
    "null tensor list": dict(tensors=None),
    "null arguments": dict(args=None),
    "null groups": dict(groups=False),
    "n == 0": dict(n=0),
    "n < 0": dict(n=-3),
    "numel == 0": dict(tensor=dict(numel=0)),
    "numel < 0": dict(tensor=dict(numel=-8)),
    "null param": dict(tensor=dict(param=None)),
    "group index below range": dict(tensor=dict(group=-1)),
    "group index past range": dict(tensor=dict(group=2), n_groups=2),
    "no groups": dict(n_groups=0),
    "more than 8 groups": dict(n_groups=9),
    "grad without exp_avg": dict(tensor=dict(exp_avg=None)),
    "grad without exp_avg_sq": dict(tensor=dict(exp_avg_sq=None)),
    "neither grad nor ema": dict(tensor=dict(grad=None, ema=None)),
}


@pytest.mark.parametrize("case", sorted(BAD_STEPS))
def test_step_argument_errors_before_any_device_call(case):
    """Each returns DAD_E_INVALID with a message.  This machine has no GPU: a device call made first would have
    returned DAD_E_HIP instead (and the made-up addresses are never read)."""
    spec = BAD_STEPS[case]
    lib = _engine.load_library()
    h = C.c_void_p()
    assert lib.dad_optim_create(C.byref(h)) == 0 and h.value
    try:
        a, keep = _args(spec.get("n_groups", 1), spec.get("groups", True))
        tensors = (DadOptimTensor * 2)(_tensor(), _tensor(**spec.get("tensor", {})))
        rc = lib.dad_optim_step(h if spec.get("handle", True) else None,
                                tensors if spec.get("tensors", True) is not None else None,
                                spec.get("n", 2),
                                C.byref(a) if spec.get("args", True) is not None else None, None)
        assert rc == DAD_E_INVALID, (case, rc)
        msg = lib.dad_last_error().decode()
        assert "optimiser step" in msg, msg
    finally:
        lib.dad_optim_destroy(h)
    del keep


def test_fused_adam_refuses_what_it_does_not_implement():
    from dynamics_aware_diffusion_amd.utils.training import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdam(p, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        FusedAdam(p, maximize=True)
    opt = FusedAdam(p, lr=3e-4)                       # construction itself needs no device
    assert set(opt.param_groups[0]) == set(torch.optim.Adam(p).param_groups[0])
    p[0].grad = torch.ones(4)
    with pytest.raises(ValueError, match="ROCm device"):      # a CPU parameter: no fallback
        opt.step()
    with pytest.raises(ValueError, match="EMA"):
        FusedAdam(p, ema_params=[])


def test_fused_adam_state_dict_is_adams():
    from dynamics_aware_diffusion_amd.utils.training import FusedAdam
    p = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2, 3))]
    adam = torch.optim.Adam(p, lr=2e-4, betas=(0.8, 0.99), weight_decay=0.01)
    for q in p:
        q.grad = torch.ones_like(q)
    adam.step()
    fused = FusedAdam(p)
    fused.load_state_dict(adam.state_dict())
    sd = fused.state_dict()
    assert sd["param_groups"] == adam.state_dict()["param_groups"]
    for i in range(2):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][i][k], adam.state_dict()["state"][i][k])
    torch.optim.Adam(p).load_state_dict(sd)


def test_cosine_annealing_warmup_closed_form():
    from dynamics_aware_diffusion_amd.utils.training import CosineAnnealingWarmup, count_parameters
    base, warmup, total, min_lr = 3e-4, 5, 20, 1e-5
    p = [torch.nn.Parameter(torch.zeros(4))]
    opt = torch.optim.SGD(p, lr=base)
    sched = CosineAnnealingWarmup(opt, warmup, total, min_lr=min_lr)
    for step in range(total + 1):
        if step < warmup:
            scale = step / warmup
        else:
            scale = 0.5 * (1.0 + math.cos(math.pi * (step - warmup) / (total - warmup)))
        want = base * scale + min_lr * (1 - scale)
        assert opt.param_groups[0]["lr"] == pytest.approx(want, rel=1e-12, abs=1e-18), step
        opt.step()
        sched.step()
    sched0 = CosineAnnealingWarmup(torch.optim.SGD(p, lr=base), warmup, total)      # min_lr = 0: base * step / warmup
    assert sched0.get_last_lr() == [0.0]
    assert count_parameters(torch.nn.Linear(3, 2)) == 8


class _Toy(torch.nn.Module):
    """What Trainer needs of a model: parameters and the five attributes its checkpoint records."""
    horizon, observation_dim, action_dim, n_timesteps, beta_schedule = 8, 3, 1, 10, "cosine"

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(4, 1)


def test_trainer_loop_checkpoint_and_ema_on_the_host(tmp_path, capsys):
    """The reference's loop with a plain torch optimiser and a custom loss (no library call): train() steps through the
    loader, update_ema moves the deep copy and bumps its versions, the checkpoint has the schema the loader reads."""
    from dynamics_aware_diffusion_amd.utils.training import EMA, Trainer
    torch.manual_seed(0)
    model = _Toy()
    loader = [{"x": torch.randn(5, 4), "y": torch.randn(5, 1)} for _ in range(3)]
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    loss_fn = lambda b: ((model.lin(b["x"]) - b["y"]) ** 2).mean()                                   # noqa: E731
    tr = Trainer(model, opt, loader, device="cpu", log_dir=str(tmp_path), save_freq=2, ema_decay=0.5, gradient_clip=1.0,
                 loss_fn=loss_fn, loss_names=["mse"])
    w0 = model.lin.weight.detach().clone()
    versions = [p._version for p in tr.ema_model.parameters()]
    tr.train(n_epochs=2)
    assert tr.global_step == 6
    assert all(p._version > v for p, v in zip(tr.ema_model.parameters(), versions))
    assert not torch.equal(model.lin.weight, w0) and not torch.equal(tr.ema_model.lin.weight, w0)
    assert not torch.equal(tr.ema_model.lin.weight, model.lin.weight)
    log = open(tmp_path / "training.log").read().splitlines()
    assert [line.split(",")[0] for line in log] == ["Epoch 1", "Epoch 2"] and all(" mse: " in line for line in log)
    saved = sorted(f for f in os.listdir(tmp_path) if f.endswith(".pt"))
    assert saved == ["checkpoint_step_2.pt", "checkpoint_step_4.pt", "checkpoint_step_6.pt"]
    ck = torch.load(tmp_path / saved[-1], weights_only=True)
    assert set(ck) == {"epoch", "global_step", "model_state_dict", "optimizer_state_dict", "config", "ema_state_dict"}
    assert ck["config"] == {"horizon": 8, "observation_dim": 3, "action_dim": 1, "n_timesteps": 10, "beta_schedule": "cosine"}
    assert "Epoch 2 Summary" in capsys.readouterr().out
    # EMA, the name-keyed class
    ema = EMA(model, decay=0.9)
    before = model.lin.weight.detach().clone()
    with torch.no_grad():
        model.lin.weight.add_(1.0)
    ema.update()
    assert torch.allclose(ema.shadow["lin.weight"], 0.9 * before + 0.1 * (before + 1.0))
    ema.apply_shadow()
    assert torch.equal(model.lin.weight, ema.shadow["lin.weight"])
    ema.restore()
    assert torch.equal(model.lin.weight, before + 1.0) and not ema.backup
