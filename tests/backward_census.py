"""Host-only census of the backward pass's kernels (manual tool, not collected by pytest; needs the built library, no device):

    python tests/backward_census.py [--quick] [--jobs N] [--case-seconds S] [--check-oracle] [--out FILE]

asks HipEngine.backward_steps (dad_debug_backward_steps: everything dad_unet_backward replays, read from its list of steps
and the per-batch geometry it launches from) what every case of a bounded space runs, records the keys below, picks a small
covering set of cases by greedy set cover (most new keys per estimated second of a test case: the float64 oracle's flops on
the CPU plus a fixed cost per case), and prints that case list and the registered conv_wgrad kernels nothing in the space
launches.  "Not reached in this space" is all it claims.  The data-gradient convs are keyed by mode 3 of
tests/forward_census.py and are left out here.

Keys of a plan (step_keys):
  ("wgrad", taps, tile, windowed)            a conv_wgrad instantiation (the domain: dad_debug_kernel_list, wgrad family), and the
  ("wgrad", taps, tile, windowed, feature)   same with `steady` (a block stages >= 2 chunks: the double-buffered loop), `part`
                                             (a part-filled last chunk behind full ones), `concat_inside` (the boundary of a
                                             channel concat inside one block's staged columns), `edge_m` / `edge_c` (a partly
                                             filled last M / C tile), `swapped` (the transposed conv: G is the input)
  ("gn", nv, padded horizon, padded groups, dtemb, short pair)      gn_mish_bwd_wave_kernel<nv>, nv = 0: gn_mish_bwd_kernel
  ("cols",)  ("bias",)  ("resid", "copy" | "add" | "to_x" | "stage")    take_cols_kernel, row_partial_sums_kernel, the identity
                                             residual (a copy, add_inplace_kernel, into d x, a staged CONV_UP data gradient)
  ("slabs", "2" .. "8" | "gt8_mod04" | "gt8_other")   sum_slabs_kernel by slab count: up to 8 its tail alone, beyond 8 the two-slab
                                             loop with equal (ksplit % 8 in {0, 4}) or unequal trips of the four thread groups
  ("colsums", "short" | "unrolled" | "unrolled_tail")   col_sums_many_kernel: batch < 25, the unrolled loop alone (batch % 32
                                             == 0), the loop and its tail
  ("padcopy",)                               pad_rows_kernel x 2 and slice_rows_cols_kernel (a zero-padded horizon);
  ("slice_cols",)                            slice_cols_kernel (d x out of its padded columns otherwise)

The space (every combination unless said otherwise):
  kernel_size    3, 5, 7
  dim            32, 64, 128, 256, and 48 / 96 (run zero-padded to 64 / 128)
  dim_mults      MULTS below: one to four levels, growing, flat and shrinking (BK_COLS)
  horizon        8 .. 512, and 24 / 100 / 200 / 384 (run zero-padded)
  transition_dim 6 (ragged first layer) and dim itself (BK_RESID of the trajectory)
  batches        BATCHES (1 .. 512)
  wgrad_blocks   default (256), 1, 16, 4096
Cases the library refuses are skipped.

--check-oracle runs, for every picked case, the float64 and the fp32 oracle on the CPU and reports the fp32 oracle's own
distance on every tensor: tests/test_hip_backward_paths.py admits a case only if that is within REL / 2 everywhere.
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
BATCHES = (1, 2, 3, 5, 8, 13, 24, 32, 57, 64, 100, 128, 250, 256, 512)
WGRAD_BLOCKS = (None, 1, 16, 4096)
WGRAD_FEATURES = ("steady", "part", "concat_inside", "edge_m", "edge_c", "swapped")
GN_FORMS = (1, 2, 4, 8, 16, 0)
from tests.test_hip_train_batch import REL, T  # noqa: E402  (the gradient gate and the schedule length of the batch tests: none new)


def step_keys(rep):
    """The keys of one HipEngine.backward_steps report."""
    out = set()
    B = rep["batch"]
    for q in rep["steps"]:
        kind = q["kind"]
        if kind == "wgrad":
            base = ("wgrad", q["taps"], q["tile"], q["windowed"])
            out.add(base)
            feats = {"steady": q["chunks"] >= 2, "part": q["samples"] % q["spc"] != 0 and q["last_chunks"] > 1,
                     "concat_inside": q["concat_inside"], "edge_m": q["edge_m"], "edge_c": q["edge_c"], "swapped": q["swapped"]}
            out |= {base + (f,) for f in WGRAD_FEATURES if feats[f]}
            if q["ksplit"] > 1:
                k = q["ksplit"]
                out.add(("slabs", str(k) if k <= 8 else "gt8_mod04" if k % 8 in (0, 4) else "gt8_other"))
        elif kind == "gn":
            out.add(("gn", q["nv"], int(q["lreal"] > 0), int(q["cpg_real"] > 0), q["dtemb"], q["short_pair"]))
        elif kind == "cols":
            out.add(("cols",))
        elif kind == "bias":
            out.add(("bias",))
        elif kind == "resid":
            out.add(("resid", "to_x" if q["to_x"] else "copy" if q["write"] == "set" else "add"))
        elif kind == "dgrad" and q["write"] == "stage":
            out.add(("resid", "stage"))
    out.add(("colsums", "short" if B < 25 else "unrolled" if B % 32 == 0 else "unrolled_tail"))
    out.add(("padcopy",) if rep["padcopy"] else ("slice_cols",))
    return out


def host_engine(td, dim, mults, H, ks, wgrad_blocks=None):
    """An engine without weights: enough to plan (no device call).  Real widths / horizon: the engine pads them."""
    from dynamics_aware_diffusion_amd._engine import HipEngine, _check
    eng = HipEngine(transition_dim=td, dim=dim, channels=[dim * k for k in mults], horizon=H, n_timesteps=T, kernel_size=ks,
                    training=True)
    if wgrad_blocks is not None:
        _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, b"wgrad_blocks", int(wgrad_blocks)))
    return eng


def case_cost(td, dim, mults, H, ks, B):
    """Rough seconds of a GPU test case beyond its fixed cost: the oracle's conv flops in float64 and fp32, forward and
    backward (tests/forward_census.py::case_cost, mode 3), plus the GPU step (small beside it)."""
    from tests.forward_census import case_cost as fwd_cost
    return fwd_cost(td, dim, mults, H, ks, B, 3)


def arch_space(quick):
    for ks, dim, mults, H in itertools.product(KERNEL_SIZES, DIMS, MULTS, HORIZONS):
        if max(mults) * dim > 2048 or H % (1 << (len(mults) - 1)):
            continue
        if quick and (dim in (48, 256) or H in (16, 24, 200, 384, 512) or len(mults) == 4):
            continue
        for td in (6, dim):
            yield (td, dim, mults, H, ks)


def arch_plans(arch):
    """{frozenset of keys: (cost, case)} of one architecture: per distinct set of keys the cheapest case that reaches it."""
    from dynamics_aware_diffusion_amd._engine import DadError, _check
    td, dim, mults, H, ks = arch
    try:
        eng = host_engine(*arch)
    except (DadError, NotImplementedError, ValueError):
        return {}
    best = {}
    for wb in WGRAD_BLOCKS:
        _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, b"wgrad_blocks", 256 if wb is None else wb))
        for B in BATCHES:
            try:
                keys = frozenset(step_keys(eng.backward_steps(B)))
            except DadError:
                continue
            cost = case_cost(td, dim, mults, H, ks, B)
            if keys not in best or cost < best[keys][0]:
                best[keys] = (cost, (td, dim, mults, H, ks, B, wb))
    return best


def case_id(case):
    td, dim, mults, H, ks, B, wb = case
    return f"k{ks}_d{dim}_m{''.join(map(str, mults))}_H{H}_td{td}_B{B}" + ("" if wb is None else f"_wb{wb}")


def oracle_distances(case, seed=47):
    """{tensor: the fp32 oracle's distance from the float64 oracle} of a case, on the scales of the GPU test."""
    from tests.test_hip_backward_paths import _reference
    ref = _reference(case_id(case), *case[:6], seed)
    return ref["orc_errs"], ref["o_out"]


def main():
    from tests.forward_census import greedy_cover
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--quick", action="store_true", help="a fraction of the space (a smoke run of the tool itself)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--case-seconds", type=float, default=2.0, help="fixed cost of a case in the cover's score (more: fewer, larger cases)")
    ap.add_argument("--check-oracle", action="store_true", help="run both oracles on the picked cases: the admission condition")
    ap.add_argument("--out", default=None, help="also write the case list and the unreached kernels there, as Python literals")
    args = ap.parse_args()
    from dynamics_aware_diffusion_amd._engine import wgrad_kernels
    registered = {("wgrad",) + k for k in wgrad_kernels()}
    archs = list(arch_space(args.quick))
    best, plans = {}, 0
    with multiprocessing.Pool(args.jobs) as pool:
        for n, part in enumerate(pool.imap_unordered(arch_plans, archs, chunksize=4)):
            plans += len(part)
            for keys, (cost, case) in part.items():
                if keys not in best or cost < best[keys][0]:
                    best[keys] = (cost, case)
            if n % 200 == 0:
                print(f"  {n} / {len(archs)} architectures, {len(best)} distinct plans", file=sys.stderr, flush=True)
    reached = set().union(*best) if best else set()
    kernels = {k for k in reached if k[0] == "wgrad" and len(k) == 4}
    assert kernels <= registered, sorted(kernels - registered)
    steady = {k[:4] for k in reached if k[0] == "wgrad" and len(k) == 5 and k[4] == "steady"}
    picked, left = greedy_cover(best, reached, args.case_seconds)
    assert not left
    head = [f"# {len(archs)} architectures x {len(BATCHES)} batches x {len(WGRAD_BLOCKS)} wgrad_blocks, {len(best)} distinct key sets",
            f"# conv_wgrad kernels reached: {len(kernels)} of {len(registered)}, {len(steady)} of them with >= 2 chunks per block; "
            f"GroupNorm-backward forms: {sorted({k[1] for k in reached if k[0] == 'gn'})}; {len(reached)} keys in all",
            f"# {len(picked)} cases cover them, about {sum(c for _, _, c in picked):.0f} s of test time by the estimate"]
    lines = head + ["CASES = ["]
    for case, keys, cost in picked:
        td, dim, mults, H, ks, B, wb = case
        lines.append(f"    ({case_id(case)!r}, {td}, {dim}, {mults!r}, {H}, {ks}, {B}, {wb!r},")
        lines.append(f"     {keys!r}),")
    lines.append("]")
    lines.append("NOT_REACHED = [")
    for k in sorted(registered - kernels):
        lines.append(f"    {k!r},")
    lines.append("]")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if args.check_oracle:
        import time
        for case, _, _ in picked:
            t0 = time.time()
            errs, o_out = oracle_distances(case)
            worst = max(errs, key=errs.get)
            flag = "" if errs[worst] <= REL / 2 else "   <-- NOT ADMITTED (fp32 oracle beyond REL / 2)"
            print(f"# {case_id(case)}: fp32 oracle {errs[worst]:.2e} x max|g| ({worst}), output {o_out:.2e}, {time.time() - t0:.1f} s{flag}",
                  flush=True)


if __name__ == "__main__":
    main()
