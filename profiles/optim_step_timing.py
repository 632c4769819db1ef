#!/usr/bin/env python3
"""Time whole training steps with the two optimiser tails (the reference's Trainer.train_step, utils/training.py:144-189):

    python3 profiles/optim_step_timing.py --arch pointmaze --batch 256            # alternating fresh processes
    python3 profiles/optim_step_timing.py --arch pointmaze --batch 256 --path fused --steps 20      # one measurement

  torch   loss.backward(), clip_grad_norm_(parameters, 1.0), torch.optim.Adam(lr=3e-4).step(), the EMA loop over every
          parameter (ema.data.mul_(d).add_(p.data, alpha=1 - d)) and the version bump that makes the EMA model's engine
          see it: the baseline
  fused   loss.backward(), FusedAdam.step(): clip + Adam + EMA in the library (dad_optim_step)

Both pay the engine refresh at the next forward (dad_model_refresh_weights).  A measurement is `--steps` steps issued
back to back and drained once; it also reports the host time to issue them (the loop's wall time before the drain).
Without --path the script is a driver that never touches the GPU itself: it runs the two paths in alternating fresh
child processes, `--runs` of each, and prints every pair, the spread and whether `fused` won every pair.

    rocprofv3 --kernel-trace --stats -- python3 profiles/optim_step_timing.py --arch pointmaze --path fused --steps 20

gives launches per step and the two kernels' own time (optim_sqsum_kernel, optim_update_kernel)."""
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
ap.add_argument("--arch", default="pointmaze")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--dim", type=int, default=0, help="override the architecture's dim")
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--steps", type=int, default=30, help="steps of the timed back-to-back loop")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--path", choices=("torch", "fused"), help="measure this path in this process (default: drive both)")
ap.add_argument("--runs", type=int, default=3, help="driver: fresh processes per path")
ap.add_argument("--child-timeout", type=float, default=240.0, help="driver: seconds one child may take")
ap.add_argument("--no-fused-objective", action="store_true", help="GaussianDiffusion.fused_objective = False")
args = ap.parse_args()


def measure():
    import copy

    import torch
    from torch.autograd.graph import increment_version

    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    from dynamics_aware_diffusion_amd.utils import synth
    from dynamics_aware_diffusion_amd.utils.training import FusedAdam

    dev = torch.device("cuda:0")
    od, ad, dim, mults, T = synth.ARCHS[args.arch]
    dim = args.dim or dim
    H, td = args.horizon, od + ad
    unet = TemporalUnet(td, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=0).items()})
    diff = GaussianDiffusion(unet, H, od, ad, n_timesteps=T).to(dev)
    diff.fused_objective = not args.no_fused_objective
    ema = copy.deepcopy(diff)
    params, ema_params = list(diff.parameters()), list(ema.parameters())
    x0 = torch.from_numpy(synth.normal_like(3, "train.x0", (args.batch, H, td))).to(dev).clamp(-1, 1)
    decay, clip, lr = 0.995, 1.0, 3e-4
    if args.path == "fused":
        opt = FusedAdam(params, lr=lr, max_grad_norm=clip, ema_params=ema_params, ema_decay=decay)

        def step():
            opt.zero_grad(set_to_none=True)
            diff.loss(x0).backward()
            opt.step()
    else:
        opt = torch.optim.Adam(params, lr=lr)

        def step():
            opt.zero_grad(set_to_none=True)
            diff.loss(x0).backward()
            torch.nn.utils.clip_grad_norm_(params, clip)
            opt.step()
            with torch.no_grad():
                for e, p in zip(ema_params, params):
                    e.data.mul_(decay).add_(p.data, alpha=1 - decay)
                increment_version(ema_params)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    n = sum(p.numel() for p in params)
    print(json.dumps({"path": args.path, "arch": args.arch, "dim": dim, "batch": args.batch, "steps": args.steps,
                      "fused_objective": diff.fused_objective, "parameters": n, "tensors": len(params),
                      "step_ms": (t2 - t0) / args.steps * 1e3, "issue_ms": (t1 - t0) / args.steps * 1e3}), flush=True)


def drive():
    base = [sys.executable, os.path.abspath(__file__), "--arch", args.arch, "--batch", str(args.batch), "--dim", str(args.dim),
            "--horizon", str(args.horizon), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    if args.no_fused_objective:
        base.append("--no-fused-objective")
    results = {"torch": [], "fused": []}
    for run in range(args.runs):
        for path in ("torch", "fused"):
            out = subprocess.run(base + ["--path", path], capture_output=True, text=True, timeout=args.child_timeout)
            if out.returncode != 0:             # a child that failed ends the whole measurement
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(f"{path} run {run} ended with status {out.returncode}")
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            results[path].append(rec)
            print(json.dumps(rec), flush=True)
    summary = {"arch": args.arch, "dim": results["torch"][0]["dim"], "batch": args.batch, "runs": args.runs,
               "parameters": results["torch"][0]["parameters"], "tensors": results["torch"][0]["tensors"]}
    for path, recs in results.items():
        for key in ("step_ms", "issue_ms"):
            v = [r[key] for r in recs]
            summary[f"{path}_{key}"] = {"min": min(v), "median": statistics.median(v), "max": max(v)}
    pairs = [t["step_ms"] / f["step_ms"] for t, f in zip(results["torch"], results["fused"])]
    summary["torch_over_fused_per_pair"] = pairs
    summary["fused_faster_in_every_pair"] = all(r > 1.0 for r in pairs)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    measure() if args.path else drive()
