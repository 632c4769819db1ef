"""Time per plan of the ancestral loop and of the K-step strided (DDIM) loop, on the flagship nets.

One process per configuration (``--config NAME`` runs that one; without it every configuration runs in a child process
of its own and the JSON lines are collected).  Inside a process the two samplers alternate, round by round, on the same
engine: both are warmed up first (which also captures the graphs of the batch-1 configuration, so capture is outside
every timed window), each timed window ends in a device synchronise, a window of the K-step loop repeats it until it
lasts about as long as 0.2 s, and the figures are medians over the rounds with the spread (max - min) / median of the
identical repeats next to them.  A third loop goes round with them: the ancestral sampler truncated to K steps
(``n_timesteps = K``, what the reference's --sampling-timesteps does), which launches exactly what the K-step strided
loop launches — it tells a cost of short loops from a cost of the strided sampler.  In-kernel Philox noise, one shared
inpainting condition, synthetic weights: timing does not depend on the values.

    python profiles/sampler_timing.py [--config NAME] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (architecture of utils/synth.ARCHS, horizon, batch, use_graph, K)
CONFIGS = {
    "pointmaze_b256_k10": ("pointmaze", 32, 256, False, 10),
    "pointmaze_b256_k20": ("pointmaze", 32, 256, False, 20),
    "halfcheetah_b1_k20": ("halfcheetah", 32, 1, True, 20),
    "halfcheetah_b1_k50": ("halfcheetah", 32, 1, True, 50),
    "door_b128_k50": ("door", 32, 128, False, 50),
}


def run_config(name):
    import torch
    from dynamics_aware_diffusion_amd import GaussianDiffusion, GuidedPolicy, TemporalUnet
    from dynamics_aware_diffusion_amd.utils import synth
    arch, H, B, graph, K = CONFIGS[name]
    od, ad, dim, mults, T = synth.ARCHS[arch]
    td = od + ad
    dev = torch.device("cuda:0")
    unet = TemporalUnet(td, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=0).items()})
    diff = GaussianDiffusion(unet, H, od, ad, n_timesteps=T).to(dev)
    diff.sampler_rng, diff.seed, diff.use_graph = "philox", 1, graph
    pol = GuidedPolicy(diff, None)
    cond = {0: torch.zeros(1, td, device=dev)}

    def window(kind, repeats):
        diff.n_timesteps = K if kind == "truncated" else T
        if kind == "ddim":
            diff.set_sampler("ddim", steps=K, eta=0.0)
        else:
            diff.set_sampler("ddpm")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            pol.sample_loop(batch_size=B, conditions=cond)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / repeats

    for kind in ("ddpm", "ddim", "truncated") * 2:         # warm-up: code objects, workspaces, graph capture
        window(kind, 1)
    t_ddpm = window("ddpm", 1)
    t_ddim = window("ddim", 3)
    rounds = max(3, min(9, int(10.0 / t_ddpm)))
    rep_ddim = max(1, int(round(0.2 / t_ddim)))
    rep_ddpm = max(1, int(round(0.2 / t_ddpm)))
    loops = {"ddpm": [], "ddim": [], "truncated": []}
    for _ in range(rounds):
        loops["ddpm"].append(window("ddpm", rep_ddpm))
        loops["ddim"].append(window("ddim", rep_ddim))
        loops["truncated"].append(window("truncated", rep_ddim))
    out = {"config": name, "arch": arch, "B": B, "H": H, "T": T, "K": K, "use_graph": graph, "rounds": rounds,
           "repeats_per_window": {"ddpm": rep_ddpm, "ddim": rep_ddim}}
    for kind, steps in (("ddpm", T), ("ddim", K), ("truncated", K)):
        med = statistics.median(loops[kind])
        out[kind] = {"ms_per_loop": 1e3 * med, "ms_per_step": 1e3 * med / steps,
                     "spread": (max(loops[kind]) - min(loops[kind])) / med}
    out["per_step_ratio"] = out["ddpm"]["ms_per_step"] / out["ddim"]["ms_per_step"]
    out["speedup_per_plan"] = out["ddpm"]["ms_per_loop"] / out["ddim"]["ms_per_loop"]
    eng = diff._engine(dev)
    out["seam"] = eng.seam_plan(B)["reason"]
    out["final"] = eng.forward_plan(B, 0)["final"][2]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.config:
        lines = [json.dumps(run_config(args.config))]
    else:
        lines = []
        for name in CONFIGS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", name], capture_output=True,
                               text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"{name}: exit status {r.returncode}")
            lines.append(r.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
    if args.config:
        print(lines[0], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
