"""Host-only census of the forward kernels (manual tool, not collected by pytest; needs the built library, no device):

    python tests/forward_census.py [--quick] [--jobs N] [--case-seconds S] [--out FILE]

asks HipEngine.forward_plan (dad_debug_forward_plan: the description the entry points replay) what every case of a
bounded space launches, records every kernel key reached — ("gemm", tile, taps, stride, flag word) of kernel_registered,
("cc", ...) / ("ccw", ...) of the small-batch kernels — and the path features tests/test_hip_forward_paths.py lists,
picks a small covering set of cases by greedy set cover (most new keys per estimated second of a test case: the float64
oracle's flops plus a fixed cost per case, so small nets and batches win), and prints that case list and the registered
kernels nothing in the space reaches.  "Not reached in this space" is all it claims: a kernel on that list may be
reachable from outside the space.

The space (every combination unless said otherwise):
  kernel_size    3, 5, 7
  dim            32, 64, 128, 256, and 48 / 96 (run zero-padded to 64 / 128)
  dim_mults      MULTS below: one to four levels, growing, flat and shrinking, widest level <= 2048 channels
  horizon        8, 16, 32, 64, 128, 256, 512, and 24 / 100 / 200 / 384 (run zero-padded to 32 / 128 / 256 / 512)
  transition_dim 6 (ragged first layer), 64 (whole chunks), and dim itself (the first block's residual is the trajectory)
  precision      fp32 (modes 0 .. 3), f16x3 (modes 0, 1: it does not train)
  modes          0 shared-timestep forward, 1 per-row timesteps, 2 training forward, 3 data-gradient convs
  batches        HEURISTIC_BATCHES under the heuristic (tile -1 and 99), FORCED_BATCHES under a forced tile
  tiles          -1, 0 .. 9, 99, 100 .. 109
  options        one at a time off their defaults (OPTION_SETS): fuse_residual 0, split_target 64 / 1024 (these two under
                 the heuristic's tiles only), and for mode 0
                 at SMALL_BATCHES: cc 0, cc_max_rows 4096, ccw_max_rows 4096 (with cc_max_rows 4096), ccw_min_blocks 1 / 4096,
                 ccw_prefer16 0
Cases the library refuses are skipped.
"""
import argparse
import itertools
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNEL_SIZES = (3, 5, 7)
DIMS = (32, 64, 128, 256, 48, 96)
MULTS = ((1,), (1, 1), (1, 2), (1, 4), (1, 8), (1, 2, 4), (1, 4, 8), (1, 1, 2), (1, 4, 2), (1, 2, 4, 8), (1, 2, 2, 4), (1, 4, 2, 1))
HORIZONS = (8, 16, 32, 64, 128, 256, 512, 24, 100, 200, 384)
HEURISTIC_BATCHES = (1, 2, 3, 4, 5, 8, 13, 16, 31, 32, 33, 64, 100, 128, 256, 512)
FORCED_BATCHES = (1, 3, 32, 256)
SMALL_BATCHES = (1, 2, 3, 4, 5, 8, 13, 16)
TILES = (-1,) + tuple(range(10)) + (99,) + tuple(range(100, 110))
OPTION_DEFAULTS = {"fuse_residual": 1, "split_target": 256, "cc": 1, "cc_max_rows": 512, "ccw_max_rows": 128, "ccw_min_blocks": 256,
                   "ccw_prefer16": 1}
OPTION_SETS = ({}, {"fuse_residual": 0}, {"split_target": 64}, {"split_target": 1024})
SMALL_OPTION_SETS = ({"cc": 0}, {"cc_max_rows": 4096}, {"cc_max_rows": 4096, "ccw_max_rows": 4096}, {"ccw_min_blocks": 1},
                     {"ccw_min_blocks": 4096}, {"ccw_prefer16": 0})
T = 20


def features(plan):
    """The path features of one plan that the matrix must cover besides the kernels themselves."""
    out = set()
    if plan["final"][1] > 1:
        out.add(("final_gy>1", plan["final"][2]))
    if plan["final"][2] == "final_cc_kernel":
        out.add(("final_cc",))
    for q in plan["launches"]:
        if plan["small"]:
            out.add(("res_kind", q["res_kind"]))
            if q["big"]:
                out.add(("big", q["tile_rows"]))
            if q["ride_in"]:
                out.add(("ride_in", q["tile_rows"]))
        else:
            out.add(("split", q["cfg"], int(q["kslices"] > 1)))
            if q["gn_npt"]:
                out.add(("gn_npt", q["gn_npt"]))
            if q["part_tile"]:
                out.add(("part_tile", q["cfg"]))
    return out


def plan_keys(plan):
    return {q["key"] for q in plan["launches"]} | features(plan)


def host_engine(td, dim, mults, H, ks, precision):
    """An engine without weights: enough to plan (no device call).  Real widths / horizon: the engine pads them."""
    from dynamics_aware_diffusion_amd._engine import HipEngine
    return HipEngine(transition_dim=td, dim=dim, channels=[dim * k for k in mults], horizon=H, n_timesteps=T, kernel_size=ks,
                     precision=precision, training=precision == "fp32")


def set_options(eng, tile, options):
    """Through the library directly: HipEngine.debug_set_* enter the device's context."""
    from dynamics_aware_diffusion_amd._engine import _check
    _check(eng.lib, eng.lib.dad_debug_set_tile(eng._h, int(tile)))
    for name, default in OPTION_DEFAULTS.items():
        _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, name.encode(), int(options.get(name, default))))


def case_cost(td, dim, mults, H, ks, B, mode):
    """Rough seconds of a GPU test case beyond its fixed cost: the float64 oracle's conv flops (twice, with its fp32 run;
    three more passes for gradients) at ~4 GFLOP/s."""
    from dynamics_aware_diffusion_amd.utils.padding import padded_width
    ch = [padded_width(dim * k) for k in mults]
    flops, L, cin = 0.0, H, td
    for i, c in enumerate(ch):
        flops += 2.0 * L * ks * (cin * c + 3 * c * c)
        cin = c
        if i < len(ch) - 1:
            L //= 2
    flops += 2.0 * L * ks * 4 * ch[-1] * ch[-1]
    for i in range(len(ch) - 1, 0, -1):
        flops += 2.0 * L * ks * (2 * ch[i] * ch[i - 1] + 3 * ch[i - 1] * ch[i - 1])
        L *= 2
    return flops * B * (2 if mode < 3 else 8) / 4e9


def arch_space(quick):
    for ks, dim, mults, H in itertools.product(KERNEL_SIZES, DIMS, MULTS, HORIZONS):
        if max(mults) * dim > 2048 or H % (1 << (len(mults) - 1)):
            continue
        if quick and (dim in (48, 256) or H in (16, 24, 200, 384, 512) or len(mults) == 4):
            continue
        for td in (6, 64, dim):
            for precision in ("fp32", "f16x3"):
                yield (td, dim, mults, H, ks, precision)


def arch_plans(arch):
    """{frozenset of keys: (cost, case)} of one architecture: per distinct set of keys the cheapest case that reaches it."""
    from dynamics_aware_diffusion_amd._engine import DadError
    td, dim, mults, H, ks, precision = arch
    try:
        eng = host_engine(*arch)
    except (DadError, NotImplementedError, ValueError):
        return {}
    best = {}
    modes = (0, 1, 2, 3) if precision == "fp32" else (0, 1)

    def visit(tile, options, batches, which):
        set_options(eng, tile, options)
        for B in batches:
            for mode in which:
                try:
                    keys = frozenset(plan_keys(eng.forward_plan(B, mode)))
                except DadError:
                    continue
                cost = case_cost(td, dim, mults, H, ks, B, mode)
                if keys and (keys not in best or cost < best[keys][0]):
                    best[keys] = (cost, (td, dim, mults, H, ks, precision, B, mode, tile, dict(options)))

    for tile in TILES:
        for options in OPTION_SETS:
            if "split_target" in options and tile != -1:
                continue                       # (aimed under the heuristic only; 99 / 100+: no grid split-K to aim)
            visit(tile, options, HEURISTIC_BATCHES if tile in (-1, 99) else FORCED_BATCHES, modes)
    if precision == "fp32":
        for options in SMALL_OPTION_SETS:
            visit(-1, options, SMALL_BATCHES + ((32, 64, 128) if "cc_max_rows" in options else ()), (0,))
    return best


def greedy_cover(best, universe, case_seconds):
    """[(case, the keys it is picked for, its cost)]: repeatedly the case with the most uncovered keys per second of cost
    (`case_seconds`: what every case costs whatever its size — building the engine, packing weights, starting the oracle)."""
    left = set(universe)
    picked = []
    items = [(keys & universe, case_seconds + cost, case) for keys, (cost, case) in best.items()]
    while left:
        score, choice = 0.0, None
        for keys, cost, case in items:
            n = len(keys & left)
            if n and (n / cost > score or (n / cost == score and choice is not None and cost < choice[1])):
                score, choice = n / cost, (keys, cost, case)
        if choice is None:
            break
        new = choice[0] & left
        picked.append((choice[2], sorted(new), choice[1]))
        left -= new
    return picked, left


def case_id(case):
    td, dim, mults, H, ks, precision, B, mode, tile, options = case
    opt = "".join(f"_{k}{v}" for k, v in sorted(options.items()))
    return f"k{ks}_d{dim}_m{''.join(map(str, mults))}_H{H}_td{td}_{precision}_B{B}_mode{mode}_t{tile}{opt}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--quick", action="store_true", help="a fraction of the space (a smoke run of the tool itself)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--case-seconds", type=float, default=8.0, help="fixed cost of a case in the cover's score (more: fewer, larger cases)")
    ap.add_argument("--out", default=None, help="also write the case list and the unreached kernels there, as Python literals")
    args = ap.parse_args()
    from dynamics_aware_diffusion_amd._engine import registered_kernels
    gemm, cc, ccw = registered_kernels()
    archs = list(arch_space(args.quick))
    best = {}
    with multiprocessing.Pool(args.jobs) as pool:
        for n, part in enumerate(pool.imap_unordered(arch_plans, archs, chunksize=4)):
            for keys, (cost, case) in part.items():
                if keys not in best or cost < best[keys][0]:
                    best[keys] = (cost, case)
            if n % 200 == 0:
                print(f"  {n} / {len(archs)} architectures, {len(best)} distinct plans", file=sys.stderr, flush=True)
    reached = set().union(*best) if best else set()
    registered = gemm | cc | ccw
    stray = sorted(k for k in reached if k[0] in ("gemm", "cc", "ccw") and k not in registered)
    assert not stray, f"plans name kernels outside the registered domain: {stray}"
    feats = {k for k in reached if k[0] not in ("gemm", "cc", "ccw")}
    picked, left = greedy_cover(best, (reached & registered) | feats, args.case_seconds)
    assert not left
    not_reached = sorted(registered - reached)
    print(f"# {len(archs)} architectures, {len(best)} distinct plans")
    print(f"# conv-GEMM kernels reached: {len(reached & gemm)} of {len(gemm)}; conv_cc: {len(reached & cc)} of {len(cc)}; "
          f"conv_ccw: {len(reached & ccw)} of {len(ccw)}; path features: {len(feats)}")
    print(f"# {len(picked)} cases cover them, about {sum(c for _, _, c in picked):.0f} s of test time by the estimate")
    lines = [f"# conv-GEMM kernels reached: {len(reached & gemm)} of {len(gemm)}; conv_cc: {len(reached & cc)} of {len(cc)}; "
             f"conv_ccw: {len(reached & ccw)} of {len(ccw)}", "CASES = ["]
    for case, keys, cost in picked:
        td, dim, mults, H, ks, precision, B, mode, tile, options = case
        lines.append(f"    ({case_id(case)!r}, {td}, {dim}, {mults!r}, {H}, {ks}, {precision!r}, {B}, {mode}, {tile}, {options!r},")
        lines.append(f"     {keys!r}),")
    lines.append("]")
    lines.append("# registered kernels not reached in this space (not a claim that they are dead)")
    lines.append("NOT_REACHED = [")
    for k in not_reached:
        lines.append(f"    {k!r},")
    lines.append("]")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
