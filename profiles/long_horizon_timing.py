"""Horizons above 128 positions (windowed conv tiles + the GroupNorm pass): time per denoise step of whole sampling
loops and per forward of level-0-only nets, against the same work at 128 positions.

    python profiles/long_horizon_timing.py            # loops + level-0 comparison
    python profiles/long_horizon_timing.py --layers   # only the level-0 nets at H = 256 (for a rocprofv3 run)

Level-0-only nets (dim_mults = (1,)) run every conv at the horizon's length; at H = 128 with twice the batch they do
the same FLOPs on whole-sample tiles, which is the yardstick for the windowed route."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dynamics_aware_diffusion_amd import GaussianDiffusion, GuidedPolicy, TemporalUnet  # noqa: E402
from dynamics_aware_diffusion_amd.utils import synth  # noqa: E402

dev = torch.device("cuda:0")


def make(td, dim, mults, H, T):
    unet = TemporalUnet(td, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=0).items()})
    return GaussianDiffusion(unet, H, 4, td - 4, n_timesteps=T).to(dev)


def loop(label, td, dim, mults, H, B, T=100):
    diff = make(td, dim, mults, H, T)
    diff.sampler_rng, diff.seed, diff.use_graph = "philox", 1, B == 1
    pol = GuidedPolicy(diff, None)
    cond = {0: torch.zeros(1, td, device=dev)}
    pol.sample_loop(batch_size=B, conditions=cond)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        pol.sample_loop(batch_size=B, conditions=cond)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    f = synth.unet_flops_per_sample(td, dim, mults, H) * B
    print(f"{label} H={H} B={B}: {best / T * 1e6:.1f} us per denoise step, {f * T / best / 1e12:.1f} TFLOP/s", flush=True)


def forward(label, td, dim, H, B, reps=50):
    mults = (1,)
    diff = make(td, dim, mults, H, 100)
    x = torch.randn(B, H, td, device=dev)
    torch.set_grad_enabled(False)                     # the sampling engine (no autograd graph)
    for _ in range(3):
        diff.model(x, 7)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        diff.model(x, 7)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    f = synth.unet_flops_per_sample(td, dim, mults, H) * B
    print(f"{label} level-0 net dim {dim} H={H} B={B}: {us:.1f} us per forward, {f / us / 1e6:.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", action="store_true")
    args = ap.parse_args()
    if args.layers:
        forward("windowed", 6, 128, 256, 128, reps=20)
        sys.exit(0)
    for dim, rows in ((128, 32768), (128, 8192)):
        for H in (128, 256, 512):
            forward("windowed" if H > 128 else "whole-sample", 6, dim, H, rows // H)
    loop("PointMaze net", 6, 128, (1, 2, 4), 128, 1)
    loop("PointMaze net", 6, 128, (1, 2, 4), 256, 1)
    loop("PointMaze net", 6, 128, (1, 2, 4), 128, 64)
    loop("PointMaze net", 6, 128, (1, 2, 4), 256, 32)
    loop("PointMaze net", 6, 128, (1, 2, 4), 512, 16)
    loop("dim 128 (1,2,4,8)", 6, 128, (1, 2, 4, 8), 128, 64)
    loop("dim 128 (1,2,4,8)", 6, 128, (1, 2, 4, 8), 256, 32)
