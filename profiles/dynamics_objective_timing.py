#!/usr/bin/env python3
"""Time whole dynamics-aware training steps — the loss as a user calls it (its device-to-host copies of the parts
included), ``backward()`` and ``FusedAdam.step()`` — three ways on the architecture's synthetic net:

    python3 profiles/dynamics_objective_timing.py                                    # driver: every point, fresh processes
    python3 profiles/dynamics_objective_timing.py --path library --arch pointmaze --batch 256        # one measurement

  composed  ComposedLoss([DiffusionLoss, PredictedProjectionLoss]): two evaluations of the denoiser per step
  default   DynamicsAwareLoss with ``fused_objective`` off: one evaluation, the existing autograd nodes
  library   DynamicsAwareLoss with ``fused_objective`` on: dad_train_dynamics_objective_forward / _backward as one node

Points: PointMaze B = 256, PointMaze with ``--dim 64`` B = 32, Door B = 128.  A measurement is ``--iters`` steps issued
back to back after ``--warmup`` steps and drained once; the driver never touches the GPU itself, runs the three paths of
a point in alternating fresh child processes, ``--runs`` of each, and prints every record, then min / median / max per
path and whether the slowest ``default`` run beats the fastest ``composed`` run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATHS = ("composed", "default", "library")
ap = argparse.ArgumentParser()
ap.add_argument("--path", choices=PATHS)
ap.add_argument("--arch", default="pointmaze")
ap.add_argument("--dim", type=int, default=0, help="the net's base width (0: the architecture's own)")
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--iters", type=int, default=None, help="steps timed (default 30; driver: the point's own count unless given)")
ap.add_argument("--warmup", type=int, default=None, help="steps before them (default 5; driver: as --iters)")
ap.add_argument("--runs", type=int, default=3, help="driver: fresh processes per path")
ap.add_argument("--child-timeout", type=float, default=240.0, help="driver: seconds one child may take")
args = ap.parse_args()
ITERS, WARMUP = 30, 5


def measure():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    from dynamics_aware_diffusion_amd.losses import ComposedLoss, DiffusionLoss, DynamicsAwareLoss, PredictedProjectionLoss
    from dynamics_aware_diffusion_amd.utils import synth
    from dynamics_aware_diffusion_amd.utils.training import FusedAdam
    dev = torch.device("cuda:0")
    od, ad, dim, mults, T = synth.ARCHS[args.arch]
    dim = args.dim or dim
    H, td, B = args.horizon, od + ad, args.batch
    unet = TemporalUnet(td, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=0).items()})
    diff = GaussianDiffusion(unet, H, od, ad, n_timesteps=T).to(dev)
    g = torch.Generator().manual_seed(0)
    D = (H + 1) * od + H * ad
    P = torch.randn(D, D, generator=g) / D ** 0.5

    class Norm:
        obs_mean, obs_std = torch.randn(od, generator=g).numpy(), (0.5 + torch.rand(od, generator=g)).numpy()
        action_mean, action_std = torch.randn(ad, generator=g).numpy(), (0.5 + torch.rand(ad, generator=g)).numpy()

    kw = dict(state_dim=od, action_dim=ad, observation_dim=od, horizon=H, device=str(dev))
    if args.path == "composed":
        loss_fn = ComposedLoss([DiffusionLoss(diff, 1.0), PredictedProjectionLoss(diff, P, Norm, weight=0.1, **kw)])
        route = "composed"
    else:
        diff.fused_objective = args.path == "library"
        loss_fn = DynamicsAwareLoss(diff, P, Norm, projection_weight=0.1, **kw)
        route = loss_fn.route(B)[0]
        if route != args.path:
            sys.exit(f"asked for the {args.path} route, the loss takes {loss_fn.route(B)}")
    opt = FusedAdam(list(diff.parameters()), lr=1e-5)
    batch = {"conditions": torch.from_numpy(synth.normal_like(3, "train.x0", (B, H, td))).to(dev).clamp(-1, 1)}

    def step():
        total, _ = loss_fn(batch)
        opt.zero_grad()
        total.backward()
        opt.step()

    iters, warmup = args.iters or ITERS, WARMUP if args.warmup is None else args.warmup
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    print(json.dumps({"path": args.path, "route": route, "arch": args.arch, "dim": dim, "D": D, "batch": B, "iters": iters,
                      "ms": ms}), flush=True)


POINTS = [
    {"arch": "pointmaze", "batch": 256},
    {"arch": "pointmaze", "dim": 64, "batch": 32},
    {"arch": "door", "batch": 128, "iters": 10, "warmup": 3},
]


def drive():
    for kw in POINTS:
        kw = {"iters": ITERS, "warmup": WARMUP, **kw, "horizon": args.horizon}
        kw.update({k: v for k, v in (("iters", args.iters), ("warmup", args.warmup)) if v is not None})     # the command line wins
        base = [sys.executable, os.path.abspath(__file__)] + [s for k, v in kw.items() for s in (f"--{k}", str(v))]
        results = {p: [] for p in PATHS}
        for run in range(args.runs):
            for path in PATHS:
                out = subprocess.run(base + ["--path", path], capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:             # a child that failed ends the whole measurement
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(f"{kw} {path} run {run} ended with status {out.returncode}")
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                results[path].append(rec)
                print(json.dumps(rec), flush=True)
        summary = {**kw, "runs": args.runs}
        for path, recs in results.items():
            v = [r["ms"] for r in recs]
            summary[path + "_ms"] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
        summary["slowest_default_beats_fastest_composed"] = summary["default_ms"]["max"] < summary["composed_ms"]["min"]
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    if args.path:
        import torch
        measure()
    else:
        drive()
