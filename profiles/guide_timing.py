"""Time per guided plan: the parent commit's library (autograd guide, one engine step per iteration) against this
build's library guide (``ValueGuidedPolicy.fused_guide``, one ``dad_guided_loop`` call per plan).

The two sides run in alternating fresh processes, ``--runs`` times each per shape (a child is ``--side parent|new
--shape NAME``; the parent side loads ``--parent-lib`` through ``DAD_LIB`` and, having no guide entry points, can only
take the autograd route; the new side times the library route and, for reference, the autograd route on its own
library).  Every child runs under its own time limit; the first one that fails ends the whole run.  Inside a child:
two warm-up loops (code objects, workspaces, graph capture), then ``rounds`` timed windows, each ended by a device
synchronise and long enough to last about 0.2 s; the figure is the median window, next to (max - min) / median.  The
new side also times the guide kernel alone (HIP events around 200 back-to-back ``GuideState.grad`` launches) and
says how many launches a step of each route enqueues.  In-kernel Philox noise, one shared condition, synthetic
weights: timing does not depend on the values.

    python profiles/guide_timing.py --parent-lib /path/to/parent/libdad_hip.so [--out FILE] [--runs 3]
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

# name: (architecture of utils/synth.ARCHS, horizon, batch, use_graph, hidden widths, activation, guide_weight, entry)
SHAPES = {
    "pointmaze_guided_b256": ("pointmaze", 32, 256, False, (16,), "Tanh", 0.1, "sample_loop"),      # bench.py's guided configuration
    "pointmaze_guided_b1_graph": ("pointmaze", 32, 1, True, (16,), "Tanh", 0.1, "get_action"),
    "pointmaze_relu256_b256": ("pointmaze", 32, 256, False, (256, 256), "ReLU", 0.1, "sample_loop"),
}


def run_shape(name, side):
    import torch
    import types
    import numpy as np
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet, ValueGuidedPolicy
    from dynamics_aware_diffusion_amd.utils import synth
    arch, H, B, graph, hidden, act, gw, entry = SHAPES[name]
    od, ad, dim, mults, T = synth.ARCHS[arch]
    td = od + ad
    dev = torch.device("cuda:0")
    unet = TemporalUnet(td, dim=dim, dim_mults=mults)
    unet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=0).items()})
    diff = GaussianDiffusion(unet, H, od, ad, n_timesteps=T).to(dev)
    diff.sampler_rng, diff.seed = "philox", 1
    mods, k = [], od
    for n in hidden:
        mods += [torch.nn.Linear(k, n), getattr(torch.nn, act)()]
        k = n
    value = torch.nn.Sequential(*mods, torch.nn.Linear(k, 1)).to(dev)
    with torch.no_grad():
        for i, prm in enumerate(value.parameters()):
            bound = 0.7 if len(hidden) == 1 else 1.0 / max(prm.shape[-1], 1) ** 0.5
            prm.copy_(torch.from_numpy(synth.uniform(31, f"bench.value.{i}", tuple(prm.shape), bound)))
    norm = types.SimpleNamespace(obs_mean=np.zeros(od, np.float32), obs_std=np.ones(od, np.float32),
                                 normalize_observations=lambda o: o, unnormalize_actions=lambda a: a)
    cond = {0: torch.zeros(1, td, device=dev)}
    obs = np.zeros(od, np.float32)

    def policy(fused):
        pol = ValueGuidedPolicy(diff, norm, value, guide_weight=gw, action_horizon=0)
        pol.fused_guide = fused
        return pol

    def window(pol, repeats):
        # graph replay needs the fused loop: the stepwise route ignores use_graph, as it always has
        diff.use_graph = graph
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeats):
            if entry == "get_action":
                pol.action_buffer.clear()
                pol.get_action(obs)
            else:
                pol.sample_loop(batch_size=B, conditions=cond)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / repeats

    routes = {"autograd": policy(False)}
    if side == "new":
        routes["library"] = policy(True)
        assert routes["library"].guide_route(cond, B)[0] == "library", routes["library"].guide_route(cond, B)
    out = {"shape": name, "side": side, "B": B, "H": H, "T": T, "use_graph": graph, "value_net": [od, *hidden, 1],
           "activation": act, "entry": entry}
    with torch.no_grad():
        for pol in routes.values():
            window(pol, 2)
        first = {r: window(pol, 1) for r, pol in routes.items()}
        rounds = 5
        times = {r: [] for r in routes}
        for _ in range(rounds):
            for r, pol in routes.items():
                times[r].append(window(pol, max(1, int(round(0.2 / first[r])))))
        for r in routes:
            med = statistics.median(times[r])
            out[r] = {"ms_per_loop": 1e3 * med, "ms_per_step": 1e3 * med / T, "spread": (max(times[r]) - min(times[r])) / med}
        eng = diff._engine(dev)
        plan = eng.forward_plan(B, 0)
        seam = bool(eng.seam_plan(B)["taken"])
        convs = len(plan["launches"])
        out["launches_per_step"] = {"evaluation": convs, "autograd": f"{convs} + 1 tail + the guide's torch kernels",
                                    "library": convs + 1 + (0 if seam else 1), "seam": seam}
        if side == "new":
            state = routes["library"]._library_guide()[0]
            x = torch.randn(B, H, td, device=dev)
            for _ in range(20):
                state.grad(x)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(200):
                state.grad(x)
            e1.record()
            torch.cuda.synchronize()
            out["guide_kernel_us"] = 1e3 * e0.elapsed_time(e1) / 200
            out["guide_plan"] = state.plan(B, H, td)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--side", choices=("parent", "new"))
    ap.add_argument("--parent-lib", help="libdad_hip.so built from the parent commit")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    args = ap.parse_args()
    if args.shape:
        print(json.dumps(run_shape(args.shape, args.side)), flush=True)
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libdad_hip.so is needed")
    lines = []
    for name in SHAPES:
        for run in range(args.runs):
            for side in ("parent", "new"):
                env = dict(os.environ)
                env.pop("DAD_LIB", None)
                if side == "parent":
                    env["DAD_LIB"] = os.path.abspath(args.parent_lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--side", side], env=env,
                                   capture_output=True, text=True, timeout=args.limit)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-4000:])
                    raise SystemExit(f"{name} ({side}, run {run}): exit status {r.returncode}")
                lines.append(r.stdout.strip().splitlines()[-1])
                print(lines[-1], flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(lines[-1] + "\n")
    # the claim the runs support: slowest new run against fastest parent run, per shape, next to the parent's spread
    for name in SHAPES:
        rows = [json.loads(l) for l in lines if json.loads(l)["shape"] == name]
        parent = [r["autograd"]["ms_per_loop"] for r in rows if r["side"] == "parent"]
        new = [r["library"]["ms_per_loop"] for r in rows if r["side"] == "new"]
        summary = {"shape": name, "parent_ms": parent, "new_ms": new, "parent_spread": (max(parent) - min(parent)) / min(parent),
                   "slowest_new_over_fastest_parent": max(new) / min(parent)}
        print(json.dumps({"summary": summary}), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps({"summary": summary}) + "\n")


if __name__ == "__main__":
    main()
