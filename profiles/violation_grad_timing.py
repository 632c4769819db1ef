#!/usr/bin/env python3
"""Time the differentiable dynamics violation (dad_projection_violation_fwd / _bwd) against the same expression in
torch ops on the same device — what the reference would run (losses/__init__.py:161-186 under autograd):

    python3 profiles/violation_grad_timing.py                     # driver: every point below, fresh processes
    python3 profiles/violation_grad_timing.py --what op --n 4 --m 2 --horizon 32 --batch 256 --path gemm     # one

  op     forward + backward of the per-row violation alone (sum(w * viol).backward() on a leaf x), paths: row, gemm
         (the two forms forced), auto (the planner's choice) and torch (the yardstick)
  step   a whole composed training step: ComposedLoss([DiffusionLoss, PredictedProjectionLoss]).backward() on the
         architecture's synthetic net, paths: hip (PredictedProjectionLoss as shipped) and torch (the same term with its
         violation written in torch ops; the denoiser runs on the engine either way)

Points: PointMaze (B = 256, D = 196) and Door (B = 128, D = 2183) for both; D = 196 and D = 514 at B = 256 with both forms
for the crossover constant kViolationGemmMinD.  A measurement is `--iters` calls issued back to back after `--warmup`
calls and drained once; the driver never touches the GPU itself, runs every path of a point in alternating fresh child
processes, `--runs` of each, and prints every record, then min / median / max per path."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=("op", "step"))
ap.add_argument("--path", choices=("row", "gemm", "auto", "torch", "hip"))
ap.add_argument("--arch", default="pointmaze", help="step: the net")
ap.add_argument("--n", type=int, default=4)
ap.add_argument("--m", type=int, default=2)
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=3, help="driver: fresh processes per path")
ap.add_argument("--child-timeout", type=float, default=240.0, help="driver: seconds one child may take")
args = ap.parse_args()


def torch_violation(x, P, n, od, om, osd, am, asd):
    s = x[:, :, :n] * osd[:n] + om[:n]
    a = x[:, :, od:] * asd + am
    v = torch.cat([torch.cat([s, s[:, -1:]], dim=1).reshape(x.shape[0], -1), a.reshape(x.shape[0], -1)], dim=1)
    return ((v - v @ P) ** 2).sum(dim=1)


def timed(call):
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.iters * 1e3


def projector(n, m, H, dev):
    g = torch.Generator().manual_seed(0)
    D = (H + 1) * n + H * m
    P = (torch.randn(D, D, generator=g) / D ** 0.5).to(dev)
    stats = [t.to(dev) for t in (torch.randn(n, generator=g), 0.5 + torch.rand(n, generator=g),
                                 torch.randn(m, generator=g), 0.5 + torch.rand(m, generator=g))]
    return D, P, stats


def measure_op():
    from dynamics_aware_diffusion_amd._engine import ProjectionState
    dev = torch.device("cuda:0")
    n, m, H, B = args.n, args.m, args.horizon, args.batch
    D, P, stats = projector(n, m, H, dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, H, n + m, generator=g).to(dev).requires_grad_(True)
    w = torch.randn(B, generator=g).to(dev)
    st = ProjectionState(P, *stats, n, n, m, dev)
    form = None if args.path == "auto" else args.path

    def call():
        x.grad = None
        viol = torch_violation(x, P, n, n, *stats) if args.path == "torch" else st.violation_fn(x, form)
        (viol * w).sum().backward()

    ms = timed(call)
    taken = "torch" if args.path == "torch" else st.grad_plan(B, H, form)["form"]
    print(json.dumps({"what": "op", "path": args.path, "form": taken, "D": D, "batch": B, "iters": args.iters, "ms": ms}), flush=True)


def measure_step():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    from dynamics_aware_diffusion_amd.losses import ComposedLoss, DiffusionLoss, PredictedProjectionLoss
    from dynamics_aware_diffusion_amd.utils import synth
    dev = torch.device("cuda:0")
    od, ad, dim, mults, T = synth.ARCHS[args.arch]
    H, td, B = args.horizon, od + ad, args.batch
    unet = TemporalUnet(td, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=0).items()})
    diff = GaussianDiffusion(unet, H, od, ad, n_timesteps=T).to(dev)
    D, P, stats = projector(od, ad, H, dev)

    class Norm:
        obs_mean, obs_std, action_mean, action_std = (s.cpu().numpy() for s in stats)

    term = PredictedProjectionLoss(diff, P, Norm, state_dim=od, action_dim=ad, observation_dim=od, horizon=H, weight=0.1, device=str(dev))
    if args.path == "torch":
        term.violation = lambda x: torch_violation(x, P, od, od, *stats)
    terms = ComposedLoss([DiffusionLoss(diff, 1.0), term])
    x0 = torch.from_numpy(synth.normal_like(3, "train.x0", (B, H, td))).to(dev).clamp(-1, 1)
    params = list(diff.parameters())

    def call():                             # (no .item(): nothing drains the stream inside the window)
        for p in params:
            p.grad = None
        sum(t({"conditions": x0}) for t in terms.losses).backward()

    ms = timed(call)
    print(json.dumps({"what": "step", "path": args.path, "arch": args.arch, "D": D, "batch": B, "iters": args.iters, "ms": ms}), flush=True)


POINTS = [
    # (what, paths, arguments)
    ("op", ("row", "gemm", "torch"), {"n": 4, "m": 2, "horizon": 32, "batch": 256}),          # PointMaze, D = 196
    ("op", ("row", "gemm", "torch"), {"n": 4, "m": 2, "horizon": 85, "batch": 256}),          # D = 514: the crossover
    ("op", ("row", "gemm", "torch"), {"n": 39, "m": 28, "horizon": 32, "batch": 128}),        # Door, D = 2183
    ("step", ("hip", "torch"), {"arch": "pointmaze", "horizon": 32, "batch": 256, "iters": 30, "warmup": 5}),
    ("step", ("hip", "torch"), {"arch": "door", "horizon": 32, "batch": 128, "iters": 10, "warmup": 3}),
]


def drive():
    for what, paths, kw in POINTS:
        kw = {"iters": args.iters, "warmup": args.warmup, **kw}
        base = [sys.executable, os.path.abspath(__file__), "--what", what] + [s for k, v in kw.items() for s in (f"--{k}", str(v))]
        results = {p: [] for p in paths}
        for run in range(args.runs):
            for path in paths:
                out = subprocess.run(base + ["--path", path], capture_output=True, text=True, timeout=args.child_timeout)
                if out.returncode != 0:             # a child that failed ends the whole measurement
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(f"{what} {path} run {run} ended with status {out.returncode}")
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                results[path].append(rec)
                print(json.dumps(rec), flush=True)
        summary = {"what": what, **kw, "runs": args.runs}
        for path, recs in results.items():
            v = [r["ms"] for r in recs]
            summary[path + "_ms"] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    if args.what:
        import torch
        measure_op() if args.what == "op" else measure_step()
    else:
        drive()
