"""Host-only census of the two full-chip kernel families (manual tool, not collected by pytest; needs the built library,
no device):

    python tests/fullchip_census.py [--family halo8|seam|both] [--jobs N] [--case-seconds S] [--out FILE]

asks HipEngine.halo8_plan (dad_debug_halo8_plan) and HipEngine.seam_plan (dad_debug_seam_plan) — reports of the
description the entry points replay — what every case of a bounded space launches, turns every launch into the keys
below, picks a small covering set of cases by greedy set cover (most new keys per estimated second: the float64 oracle on
the sample subset the GPU tests run it on, ORACLE_SAMPLES, plus a cost per sample of the batch and a fixed cost per case)
and prints the case lists tests/test_hip_halo8_paths.py and tests/test_hip_seam_paths.py freeze.

conv_halo8_f32 (csrc/conv_halo8.hpp), kernel_size 5, modes 0 (shared timestep) and 1 (per-row timesteps):
  dim 32, 64, 128, 256; MULTS of tests/forward_census.py; every horizon that puts a level at 8 positions; transition_dim
  6 and dim; every batch from 128 to 4096 (a superset of "up to the batch at which every 8-position launch has taken both
  tiles": the tiles change with the batch alone); xcd_order and fuse_residual on and off.
  Keys: ("halo8", tile, ride) — the instantiation — and per launch
    ("src1", tile, ride)            a second source (the decoder's concat conv)
    ("boundary", tile, n)           the chunk at which the second source starts, n = 1, 2, 3 (3: the third or later):
                                    chunk 1 is loaded in front of the K loop, chunk 2 by its first pass, the others
                                    by the passes that follow
    ("chunks", tile, ride, n)       n = 1, 2, 3 (3: three or more) — DAD8_CHUNK's three call sites
    ("mtiles", tile, n)             M tiles
    ("wpp>1", tile)                 a (sample, group) pair spans waves
    ("res", tile) ("temb", tile)    residual operand / time embedding
    ("xcd", tile, x)                x = 1: the XCD-aware tile order; "tiles": the plain grid (y = M tile, z = N tile)
                                    the planner itself chooses under the default options, where the tiles do not
                                    deal out over the 8 XCDs (MT x NT not a multiple of 8, or no rectangle divides
                                    both); "off": the plain grid forced by the option xcd_order = 0
    ("last", tile, "part" / "full") the last N tile
    ("per_row", tile)               the time embedding indexed per sample

conv_seam_f32 (csrc/conv_seam.hpp):
  dim 32, 64, 128; horizon 8, 16, 32; transition_dim 2 .. 16; MULTS up to four levels; option "cc" on and off; every
  batch 1 .. 2048 (which holds the tile-0 / tile-1 and the "tile"-refusal boundaries wherever they lie below 2049).
  Keys: ("seam", dim, tile0) — the instantiation —, ("form", dim, tile0, H, units) and
    ("td", dim, td)                 td in SEAM_TDS (the posterior's outputs per thread depend on dim)
    ("last", H, tile0, n)           samples in the last tile, 1 .. 32 / H
    ("buffers", dim, relation)      final_act is the conv's dst, the ride's rdst, or apart from both
    ("levels", dim, n)
  and, for the CPU test only (a refused plan launches nothing of the family), the refusals that depend on the batch, at
  their boundary: SEAM_BOUNDARIES = (arch, cc, last batch taken / first batch refused or the other way round, reason).
"""
import argparse
import itertools
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.forward_census import MULTS, case_cost, greedy_cover, host_engine, set_options  # noqa: E402

HALO8_DIMS = (32, 64, 128, 256)
HALO8_BATCHES = range(128, 4097)
HALO8_OPTION_SETS = ({}, {"xcd_order": 0}, {"fuse_residual": 0}, {"xcd_order": 0, "fuse_residual": 0})
SEAM_DIMS = (32, 64, 128)
SEAM_HORIZONS = (8, 16, 32)
SEAM_TDS = (2, 8, 9, 15, 16)
SEAM_BATCHES = range(1, 2049)
ORACLE_SAMPLES = 25          # at most: three tiles of eight samples and one more (oracle_subset)
SAMPLE_SECONDS = 2e-4        # per sample of the batch: inputs, transfers, the comparison


def oracle_subset(B, spt):
    """The samples the float64 oracle is run on (samples are independent, so this is exact): every sample of the first N
    tile, of one interior tile and of the last tile (part or full), and the last sample of the tile before it.  `spt`:
    samples per tile.  Sorted, unique."""
    tiles = (B + spt - 1) // spt
    pick = set(range(min(spt, B)))
    mid = tiles // 2
    pick.update(range(mid * spt, min((mid + 1) * spt, B)))
    pick.update(range((tiles - 1) * spt, B))
    if tiles > 1:
        pick.add((tiles - 1) * spt - 1)
    return sorted(pick)


def set_all(eng, options):
    """forward_census.set_options, and the options it does not know, through the library directly."""
    from dynamics_aware_diffusion_amd._engine import _check
    set_options(eng, -1, options)
    for name in ("xcd_order", "halo8", "step_seam"):
        _check(eng.lib, eng.lib.dad_debug_set_option(eng._h, name.encode(), int(options.get(name, 1))))


# ---------------------------------------------------------------------------------------------------- halo8
def halo8_keys(records, xcd_order=1):
    out = set()
    for q in records:
        t, ride = q["cfg"], q["ride"]
        out.add(("halo8", t, ride))
        if q["src1_chunk"] >= 0:
            out.add(("src1", t, ride))
            out.add(("boundary", t, min(q["src1_chunk"], 3)))
        out.add(("chunks", t, ride, min(q["chunks"], 3)))
        out.add(("mtiles", t, q["mtiles"]))
        if q["wpp"] > 1:
            out.add(("wpp>1", t))
        if q["res"]:
            out.add(("res", t))
        if q["temb"]:
            out.add(("temb", t))
        out.add(("xcd", t, 1 if q["xcd_gn"] > 0 else "tiles" if xcd_order else "off"))
        out.add(("last", t, "part" if q["part_tile"] else "full"))
        if q["per_row"]:
            out.add(("per_row", t))
    return out


def halo8_horizons(mults):
    """Horizons whose level i (length H / 2^i) is 8 positions long for some i, and which the engine accepts."""
    n = len(mults)
    return [8 << i for i in range(n) if (8 << i) >> (n - 1) >= 4]


def halo8_space():
    for dim, mults in itertools.product(HALO8_DIMS, MULTS):
        if max(mults) * dim > 2048:
            continue
        for H in halo8_horizons(mults):
            for td in (6, dim):
                yield (td, dim, mults, H)


def halo8_arch(arch):
    from dynamics_aware_diffusion_amd._engine import DadError
    td, dim, mults, H = arch
    try:
        eng = host_engine(td, dim, mults, H, 5, "fp32")
    except (DadError, NotImplementedError, ValueError):
        return {}
    best = {}
    oracle = case_cost(td, dim, mults, H, 5, ORACLE_SAMPLES, 0)
    for options in HALO8_OPTION_SETS:
        set_all(eng, options)
        for mode in (0, 1):
            for B in HALO8_BATCHES:
                try:
                    keys = frozenset(halo8_keys(eng.halo8_plan(B, mode), options.get("xcd_order", 1)))
                except DadError:
                    continue
                cost = oracle + SAMPLE_SECONDS * B * len(mults)
                if keys and (keys not in best or cost < best[keys][0]):
                    best[keys] = (cost, (td, dim, mults, H, B, mode, dict(options)))
    return best


def halo8_case_id(case):
    td, dim, mults, H, B, mode, options = case
    opt = "".join(f"_{k}{v}" for k, v in sorted(options.items()))
    return f"d{dim}_m{''.join(map(str, mults))}_H{H}_td{td}_B{B}_mode{mode}{opt}"


# ---------------------------------------------------------------------------------------------------- seam
def seam_keys(q, dim, td, levels):
    if not q["taken"]:
        return set()
    out = {("seam", q["dim"], q["tile0"]), ("form", q["dim"], q["tile0"], 32 // q["spt"], q["units"]),
           ("last", 32 // q["spt"], q["tile0"], q["last"]), ("buffers", dim, q["buffers"]), ("levels", dim, levels)}
    if td in SEAM_TDS:
        out.add(("td", dim, td))
    return out


def seam_space():
    for dim, H, mults in itertools.product(SEAM_DIMS, SEAM_HORIZONS, MULTS):
        if H >> (len(mults) - 1) < 4:
            continue
        for td in range(2, 17):
            yield (td, dim, mults, H)


def seam_arch(arch):
    """({keys: (cost, case)}, [boundaries]) of one architecture."""
    from dynamics_aware_diffusion_amd._engine import DadError
    td, dim, mults, H = arch
    try:
        eng = host_engine(td, dim, mults, H, 5, "fp32")
    except (DadError, NotImplementedError, ValueError):
        return {}, []
    best, bounds = {}, []
    spt = 32 // H
    oracle = case_cost(td, dim, mults, H, 5, 3 * spt + 1, 0) * 5      # the oracle loop runs 5 steps
    for cc in (1, 0):
        set_all(eng, {"cc": cc})
        before = None
        for B in SEAM_BATCHES:
            try:
                q = eng.seam_plan(B, detail=True)
            except DadError:
                continue
            state = (q["reason"], q["tile"])
            if before is not None and state != before[0] and "taken" in (state[0], before[0][0]):
                bounds.append(((td, dim, mults, H), cc, before[1], B, before[0], state))
            before = (state, B)
            keys = frozenset(seam_keys(q, dim, td, len(mults)))
            cost = oracle + SAMPLE_SECONDS * 20 * B * len(mults)     # (the option product: some hundred loops)
            if keys and (keys not in best or cost < best[keys][0]):
                best[keys] = (cost, (td, dim, mults, H, B, cc))
    return best, bounds


def seam_case_id(case):
    td, dim, mults, H, B, cc = case
    return f"d{dim}_m{''.join(map(str, mults))}_H{H}_td{td}_B{B}_cc{cc}"


# ---------------------------------------------------------------------------------------------------- main
def merge(best, part):
    for keys, (cost, case) in part.items():
        if keys not in best or cost < best[keys][0]:
            best[keys] = (cost, case)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--family", choices=("halo8", "seam", "both"), default="both")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--case-seconds", type=float, default=3.0, help="fixed cost of a case in the cover's score (more: fewer, larger cases)")
    ap.add_argument("--out", default=None, help="also write the case lists there, as Python literals")
    args = ap.parse_args()
    from dynamics_aware_diffusion_amd._engine import fullchip_kernels
    reg_halo8, reg_seam = fullchip_kernels()
    lines = []
    with multiprocessing.Pool(args.jobs) as pool:
        if args.family in ("halo8", "both"):
            archs, best = list(halo8_space()), {}
            for part in pool.imap_unordered(halo8_arch, archs, chunksize=1):
                merge(best, part)
            reached = set().union(*best) if best else set()
            inst = {k for k in reached if k[0] == "halo8"}
            assert inst <= reg_halo8, f"plans name kernels outside the library's list: {sorted(inst - reg_halo8)}"
            picked, left = greedy_cover(best, reached, args.case_seconds)
            assert not left
            lines.append(f"# halo8: {len(archs)} architectures x {len(HALO8_BATCHES)} batches x {len(HALO8_OPTION_SETS)} option sets x 2 modes, "
                         f"{len(best)} distinct key sets, {len(inst)} of {len(reg_halo8)} instantiations, {len(reached) - len(inst)} features; "
                         f"{len(picked)} cases, about {sum(c for _, _, c in picked):.0f} s by the estimate")
            lines.append("HALO8_CASES = [")
            for case, keys, _ in picked:
                td, dim, mults, H, B, mode, options = case
                lines.append(f"    ({halo8_case_id(case)!r}, {td}, {dim}, {mults!r}, {H}, {B}, {mode}, {options!r},")
                lines.append(f"     {keys!r}),")
            lines += ["]", "HALO8_NOT_REACHED = ["] + [f"    {k!r}," for k in sorted(reg_halo8 - inst)] + ["]"]
            lines.append(f"HALO8_REACHED_KEYS = {sorted(reached, key=repr)!r}")
        if args.family in ("seam", "both"):
            archs, best, bounds = list(seam_space()), {}, []
            for part, b in pool.imap_unordered(seam_arch, archs, chunksize=1):
                merge(best, part)
                bounds += b
            reached = set().union(*best) if best else set()
            inst = {k for k in reached if k[0] == "seam"}
            assert inst <= reg_seam, f"plans name kernels outside the library's list: {sorted(inst - reg_seam)}"
            picked, left = greedy_cover(best, reached, args.case_seconds)
            assert not left
            lines.append(f"# seam: {len(archs)} architectures x {len(SEAM_BATCHES)} batches x cc on / off, {len(best)} distinct key sets, "
                         f"{len(inst)} of {len(reg_seam)} instantiations, {len(reached) - len(inst)} features; {len(picked)} cases, about "
                         f"{sum(c for _, _, c in picked):.0f} s by the estimate")
            lines.append("SEAM_CASES = [")
            for case, keys, _ in picked:
                td, dim, mults, H, B, cc = case
                lines.append(f"    ({seam_case_id(case)!r}, {td}, {dim}, {mults!r}, {H}, {B}, {cc},")
                lines.append(f"     {keys!r}),")
            lines += ["]", "SEAM_NOT_REACHED = ["] + [f"    {k!r}," for k in sorted(reg_seam - inst)] + ["]"]
            # one boundary per (reason change, dim, H): the cheapest architecture (td 6, fewest levels)
            seen = {}
            for arch, cc, b0, b1, s0, s1 in sorted(bounds, key=lambda b: (len(b[0][2]), b[0][2], abs(b[0][0] - 6), b[2])):
                seen.setdefault((arch[1], arch[3], cc, s0, s1), (arch, cc, b0, b1, s0, s1))
            lines.append("# (architecture, cc, last batch in the first state, first batch in the second, (reason, tile) before, after)")
            lines.append("SEAM_BOUNDARIES = [")
            lines += [f"    {b!r}," for b in seen.values()]
            lines.append("]")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
