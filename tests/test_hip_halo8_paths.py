"""Every form of the halo-skipping kernel (csrc/conv_halo8.hpp) that a plan reaches, against the float64 oracle.

tests/fullchip_census.py (a manual, host-only tool) walks kernel_size-5 nets of dim 32 .. 256 with a level at 8 positions,
every batch 128 .. 4096, both call modes and the options xcd_order / fuse_residual, asks HipEngine.halo8_plan
(dad_debug_halo8_plan: what the kernel makes of the operands each launch hands it) for every conv_halo8_f32 launch, and
picks by greedy set cover the cases frozen below as CASES: all 4 instantiations ("halo8", tile, ride) and the path
features of FEATURES.  The plain blockIdx.y / blockIdx.z grid order is a key of its own where the planner chooses it under the
default options (("xcd", tile, "tiles"): MT x NT no multiple of 8 — d64 (1, 4, 2) H32 at batch 449, 57 N tiles) and where the
option xcd_order = 0 forces it ("off").  The last case is added by hand: the first one again with xcd_order off (the same
launches in the plain order).

Host (no device): the matrix and NOT_REACHED are the library's list of the family, disjoint; every feature is reached or
listed in UNREACHED with the reason no plan reaches it; every case's keys hold on today's planner, at the first batch
that takes the form where the case relies on one.

GPU, per case: the keys on the plan the engine itself reports; unet_forward (mode 0, t = 7) or unet_forward_rows (mode 1,
timesteps drawn from utils/synth that differ between neighbouring samples, hence inside every tile, and between tiles)
with the option "halo8" on and off.  The float64 oracle runs on fullchip_census.oracle_subset — every sample of the first
N tile, of one interior tile and of the last (part or full), and the last sample of the tile before it; samples are
independent, so that is exact — under the gates of tests/test_hip_halo8.py: <= TOL_STEP from the fp32 oracle and no
farther from float64 than twice the fp32 oracle + 5e-7, the fp32 oracle itself within TOL_STEP / 2 of float64 (the
condition a case is admitted on).  Off the subset: halo8 on within TOL_STEP of halo8 off (the conv-GEMM kernels, which
tests/test_hip_forward_paths.py holds to float64), finite, and a second call gives the same bits.  The rolled-batch
property of tests/test_hip_halo8.py on a case with a two-source launch.
"""
import functools

import numpy as np
import pytest
import torch

from tests import fullchip_census as census
from tests.test_hip_parity import TOL_STEP, dev  # noqa: F401  (dev: fixture)
from tests.util import as_torch, max_abs

T = 20
# halo8: 184 architectures x 3969 batches x 4 option sets x 2 modes, 1296 distinct key sets, 4 of 4 instantiations, 46 features
# (id, transition_dim, dim, mults, horizon, batch, mode, options, the keys the case exists for)
CASES = [
    ('d64_m12_H16_td6_B889_mode1', 6, 64, (1, 2), 16, 889, 1, {},
     [('boundary', 0, 3), ('chunks', 0, 0, 2), ('chunks', 0, 1, 3), ('chunks', 1, 0, 3), ('chunks', 1, 1, 2), ('halo8', 0, 0), ('halo8', 0, 1), ('halo8', 1, 0), ('halo8', 1, 1), ('last', 0, 'part'), ('last', 1, 'part'), ('mtiles', 0, 2), ('mtiles', 1, 2), ('per_row', 0), ('per_row', 1), ('res', 0), ('res', 1), ('src1', 0, 1), ('temb', 0), ('temb', 1), ('xcd', 0, 1), ('xcd', 1, 1)]),
    ('d32_m12_H16_td6_B1792_mode0_fuse_residual0_xcd_order0', 6, 32, (1, 2), 16, 1792, 0, {'xcd_order': 0, 'fuse_residual': 0},
     [('boundary', 0, 2), ('chunks', 0, 0, 1), ('chunks', 0, 0, 3), ('chunks', 1, 0, 1), ('chunks', 1, 0, 2), ('last', 0, 'full'), ('last', 1, 'full'), ('mtiles', 0, 1), ('mtiles', 1, 1), ('src1', 0, 0), ('xcd', 0, 'off'), ('xcd', 1, 'off')]),
    ('d64_m142_H32_td6_B449_mode0', 6, 64, (1, 4, 2), 32, 449, 0, {},
     [('boundary', 1, 3), ('mtiles', 0, 4), ('mtiles', 1, 4), ('src1', 1, 0), ('xcd', 0, 'tiles'), ('xcd', 1, 'tiles')]),
    ('d64_m11_H16_td6_B1785_mode0', 6, 64, (1, 1), 16, 1785, 0, {},
     [('boundary', 1, 2), ('chunks', 1, 1, 3), ('src1', 1, 1)]),
    ('d32_m11_H16_td6_B1273_mode0', 6, 32, (1, 1), 16, 1273, 0, {},
     [('boundary', 0, 1), ('chunks', 0, 1, 2)]),
    ('d32_m18_H16_td6_B153_mode0', 6, 32, (1, 8), 16, 153, 0, {},
     [('chunks', 0, 1, 1), ('mtiles', 0, 8)]),
    ('d32_m14_H16_td6_B889_mode0', 6, 32, (1, 4), 16, 889, 0, {},
     [('chunks', 1, 1, 1)]),
    ('d32_m1421_H64_td6_B1785_mode0', 6, 32, (1, 4, 2, 1), 64, 1785, 0, {},
     [('boundary', 1, 1)]),
    ('d64_m18_H16_td6_B153_mode0', 6, 64, (1, 8), 16, 153, 0, {},
     [('mtiles', 1, 8)]),
    # by hand: the first case in the plain grid order
    ('d64_m12_H16_td6_B889_mode1_xcd_order0', 6, 64, (1, 2), 16, 889, 1, {'xcd_order': 0},
     [('halo8', 0, 0), ('halo8', 0, 1), ('halo8', 1, 0), ('halo8', 1, 1), ('per_row', 0), ('per_row', 1), ('src1', 0, 1), ('xcd', 0, 'off'), ('xcd', 1, 'off')]),
]
# instantiations of the library's list that no plan of the census space reaches
NOT_REACHED = []
# What the matrix must cover.  Tile 0 is 32 x 64 (four split-K waves per wave tile), tile 1 is 64 x 64 (two).
FEATURES = ([("halo8", t, r) for t in (0, 1) for r in (0, 1)] + [("src1", t, r) for t in (0, 1) for r in (0, 1)] +
            [("boundary", t, n) for t in (0, 1) for n in (1, 2, 3)] + [("chunks", t, r, n) for t in (0, 1) for r in (0, 1) for n in (1, 2, 3)] +
            [("mtiles", t, n) for t in (0, 1) for n in (1, 2, 4, 8)] + [("wpp>1", t) for t in (0, 1)] + [("res", t) for t in (0, 1)] +
            [("temb", t) for t in (0, 1)] + [("xcd", t, x) for t in (0, 1) for x in (1, "tiles", "off")] +
            [("last", t, f) for t in (0, 1) for f in ("part", "full")] + [("per_row", t) for t in (0, 1)])
_PAIR = ("a (sample, group) pair lies inside one block tile (tile_valid: cout / 8 <= BM), so it is owned by at most 8 positions x BM / 4 float4 "
         "over F4PL float4 per thread = 64 lanes on either tile: one wave.  The kernel's cross-wave sum (wpp > 1) is conv_gemm_f32's, kept for "
         "tiles this family does not have")
UNREACHED = {("wpp>1", 0): _PAIR, ("wpp>1", 1): _PAIR}
# (transition_dim, dim, mults, horizon, tile) -> the first batch whose default shared-timestep plan holds the family on that
# tile (None: no batch up to 4096): what the cases' batches rely on (recomputed by test_case_keys_hold_on_todays_planner)
FIRST_BATCHES = {
    (6, 64, (1, 2), 16, 0): 313, (6, 64, (1, 2), 16, 1): 889, (6, 32, (1, 2), 16, 0): 633, (6, 32, (1, 2), 16, 1): 1785,
    (6, 64, (1, 4, 2), 32, 0): 153, (6, 64, (1, 4, 2), 32, 1): 441, (6, 64, (1, 1), 16, 0): 633, (6, 64, (1, 1), 16, 1): 1785,
    (6, 32, (1, 1), 16, 0): 1273, (6, 32, (1, 1), 16, 1): None, (6, 32, (1, 8), 16, 0): 153, (6, 32, (1, 8), 16, 1): 441,
    (6, 32, (1, 4), 16, 0): 313, (6, 32, (1, 4), 16, 1): 889, (6, 32, (1, 4, 2, 1), 64, 0): 633, (6, 32, (1, 4, 2, 1), 64, 1): 1785,
    (6, 64, (1, 8), 16, 0): 633, (6, 64, (1, 8), 16, 1): 153,
}
# The plain grid the planner chooses by itself (default options, xcd_gn == 0 because MT x NT is no multiple of 8): the first
# batch of d64 (1, 4, 2) H32 at which a launch on tile 0 / tile 1 has it.  449 is the first with both: 57 N tiles x 4 M tiles.
NATURAL_PLAIN_GRID = ((6, 64, (1, 4, 2), 32), {0: 321, 1: 449})


def _host_plan(case):
    _, td, dim, mults, H, B, mode, options, _ = case
    eng = census.host_engine(td, dim, mults, H, 5, "fp32")
    census.set_all(eng, options)
    return eng.halo8_plan(B, mode)


# ------------------------------------------------------------------------------------------------ host
def test_matrix_and_not_reached_are_the_registered_instantiations():
    from dynamics_aware_diffusion_amd._engine import fullchip_kernels
    registered, _ = fullchip_kernels()
    matrix = {k for c in CASES for k in c[-1] if k[0] == "halo8"}
    assert len(registered) == 4
    assert matrix | set(NOT_REACHED) == registered and not matrix & set(NOT_REACHED)
    assert not NOT_REACHED, "every instantiation is reached"


def test_every_feature_is_reached_or_explained():
    covered = {k for c in CASES for k in c[-1]}
    assert covered <= set(FEATURES), sorted(covered - set(FEATURES))
    assert not covered & set(UNREACHED)
    assert covered | set(UNREACHED) == set(FEATURES), sorted(set(FEATURES) - covered - set(UNREACHED))
    assert len({c[0] for c in CASES}) == len(CASES)


def test_case_keys_hold_on_todays_planner():
    for case in CASES:
        plan = _host_plan(case)
        keys = census.halo8_keys(plan, case[7].get("xcd_order", 1))
        assert set(case[-1]) <= keys, (case[0], sorted(set(case[-1]) - keys))
        assert not keys & set(UNREACHED), case[0]
        # the report is of conv_halo8_f32 launches only, and names the forward plan's
        eng = census.host_engine(*case[1:5], 5, "fp32")
        census.set_all(eng, case[7])
        fwd = [q for q in eng.forward_plan(case[5], case[6])["launches"] if q["key"][0] == "halo8"]
        assert [(q["conv"], q["key"][1], q["key"][2], q["mtiles"], q["ntiles_n"], q["part_tile"]) for q in fwd] == \
               [(q["conv"], q["cfg"], q["ride"], q["mtiles"], q["ntiles_n"], q["part_tile"]) for q in plan], case[0]
    for (td, dim, mults, H, tile), first in FIRST_BATCHES.items():
        eng = census.host_engine(td, dim, mults, H, 5, "fp32")
        census.set_all(eng, {})
        took = lambda B: any(q["cfg"] == tile for q in eng.halo8_plan(B, 0))
        if first is None:
            assert not any(took(B) for B in range(128, 4097)), (dim, mults, H, tile)
        else:
            assert took(first) and not any(took(B) for B in range(1, first)), (dim, mults, H, tile, first)
    assert {c[1:5] for c in CASES} == {k[:4] for k in FIRST_BATCHES}
    arch, firsts = NATURAL_PLAIN_GRID
    eng = census.host_engine(*arch, 5, "fp32")
    census.set_all(eng, {})
    for tile, first in firsts.items():
        plain = lambda B: ("xcd", tile, "tiles") in census.halo8_keys(eng.halo8_plan(B, 0))
        assert plain(first) and not any(plain(B) for B in range(1, first)), (tile, first)
    case = next(c for c in CASES if ("xcd", 0, "tiles") in c[-1])
    assert case[1:5] == arch and case[7] == {} and case[5] == max(firsts.values())
    plan = _host_plan(case)
    assert plan and all(q["xcd_gn"] == 0 and (q["mtiles"] * q["ntiles_n"]) % 8 != 0 for q in plan), "every launch of it runs the plain grid"
    assert {q["cfg"] for q in plan} == {0, 1}
    # the subset the oracle runs on: whole first, interior and last tiles and the sample in front of the last tile
    for B in (153, 313, 889, 1792):
        sub = census.oracle_subset(B, 8)
        tiles = (B + 7) // 8
        assert sub == sorted(set(sub)) and set(range(8)) <= set(sub) and set(range((tiles - 1) * 8, B)) <= set(sub)
        assert (tiles - 1) * 8 - 1 in sub and set(range(tiles // 2 * 8, tiles // 2 * 8 + 8)) <= set(sub) and len(sub) <= census.ORACLE_SAMPLES
        assert 0 < tiles // 2 < tiles - 1


# ------------------------------------------------------------------------------------------------ GPU
def _timesteps(name, B):
    """One timestep per sample, drawn from utils/synth; neighbours differ (so every tile of eight holds several)."""
    from dynamics_aware_diffusion_amd.utils import synth
    t = np.floor((synth.uniform(59, "halo8p.t." + name, (B,), 1.0).astype(np.float64) + 1.0) * 0.5 * T).astype(np.int64) % T
    for b in range(1, B):
        if t[b] == t[b - 1]:
            t[b] = (t[b] + 1 + b % (T - 2)) % T
            if t[b] == t[b - 1]:
                t[b] = (t[b] + 1) % T
    return t


@functools.lru_cache(maxsize=None)
def _reference(net_id, td, dim, mults, H, B, mode):
    """Weights, input, timesteps and the oracle's fp32 / float64 forward on the subset; nobody writes into it.  Cases that
    differ in options only share it (`net_id`: the id without the options)."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    state = synth.synth_unet_state(td, dim, mults, seed=61, affine_jitter=0.3)
    w = as_torch(state)
    x = torch.from_numpy(synth.normal_like(29, "halo8p.x." + net_id, (B, H, td)))
    t = torch.from_numpy(_timesteps(net_id, B)) if mode == 1 else torch.full((B,), 7, dtype=torch.long)
    sub = census.oracle_subset(B, 8)
    with torch.no_grad():
        out32 = orc.unet_forward(w, x[sub], t[sub]).numpy()
        out64 = orc.unet_forward(orc.cast_weights(w, torch.float64), x[sub].double(), t[sub]).numpy()
    return {"state": state, "x": x, "t": t, "sub": sub, "out32": out32, "out64": out64, "o64": max_abs(out32, out64)}


def _net_id(case):
    name, td, dim, mults, H, B, mode, _, _ = case
    return f"d{dim}_m{''.join(map(str, mults))}_H{H}_td{td}_B{B}_mode{mode}"


def _forward(eng, ref, mode, dev, x=None):
    x = ref["x"].to(dev) if x is None else x
    return eng.unet_forward_rows(x, ref["t"].to(dev)) if mode == 1 else eng.unet_forward(x, 7)


def _set(eng, options):
    for k in ("xcd_order", "fuse_residual"):
        eng.debug_set_option(k, options.get(k, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_halo8_case_vs_float64(case, dev):
    from tests.test_hip_long_horizon import _diffusion
    name, td, dim, mults, H, B, mode, options, keys = case
    ref = _reference(_net_id(case), td, dim, mults, H, B, mode)
    if mode == 1:
        tt = ref["t"].numpy()
        assert (tt[1:] != tt[:-1]).all() and len({tuple(tt[i:i + 8]) for i in range(0, B - 8, 8)}) > 1
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, ref["state"], dev)
    eng = diff.model.engine(H, dev)
    got = {}
    try:
        _set(eng, options)
        for on in (1, 0):
            eng.debug_set_option("halo8", on)
            plan = eng.halo8_plan(B, mode)
            if on:
                have = census.halo8_keys(plan, options.get("xcd_order", 1))
                assert set(keys) <= have, (name, sorted(set(keys) - have))
            else:
                assert not plan, name
            got[on] = _forward(eng, ref, mode, dev).cpu().numpy()
            if on:
                assert np.array_equal(got[on], _forward(eng, ref, mode, dev).cpu().numpy()), "a second call gives other bits"
            assert diff.model._engine is eng
    finally:
        eng.debug_set_option("halo8", 1)
        _set(eng, {})
    sub = ref["sub"]
    assert ref["o64"] <= TOL_STEP / 2, f"{name}: the fp32 oracle is {ref['o64']:.2e} from float64: the gate could not tell a wrong kernel from fp32"
    for on in (1, 0):
        e32, e64 = max_abs(got[on][sub], ref["out32"]), max_abs(got[on][sub], ref["out64"])
        print(f"\n{name} halo8={on}: on {len(sub)} samples |hip-orc32|={e32:.2e} |hip-fp64|={e64:.2e} |orc32-fp64|={ref['o64']:.2e}")
        assert np.isfinite(got[on]).all()
        assert e32 <= TOL_STEP, (name, on)
        assert e64 <= 2 * ref["o64"] + 5e-7, (name, on)
    rest = max_abs(got[1], got[0])
    print(f"{name}: |halo8 - conv-GEMM| over the whole batch = {rest:.2e}")
    assert rest <= TOL_STEP, name


@pytest.mark.gpu
def test_halo8_two_source_result_does_not_depend_on_the_column_of_a_sample(dev):
    """A sample gives the same bits in whichever column of whichever tile it sits (rolled batch), in a partly empty last
    tile, with per-row timesteps rolled along: the first case, whose decoder conv reads two sources and carries the
    ride."""
    from tests.test_hip_long_horizon import _diffusion
    case = CASES[0]
    name, td, dim, mults, H, B, mode, options, keys = case
    assert ("src1", 0, 1) in keys and mode == 1
    ref = _reference(_net_id(case), td, dim, mults, H, B, mode)
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, ref["state"], dev)
    eng = diff.model.engine(H, dev)
    assert ("src1", 0, 1) in census.halo8_keys(eng.halo8_plan(B, mode))
    x, t = ref["x"].to(dev), ref["t"].to(dev)
    a = eng.unet_forward_rows(x, t)
    b = eng.unet_forward_rows(torch.roll(x, 5, 0).contiguous(), torch.roll(t, 5, 0).contiguous())
    assert torch.equal(torch.roll(a, 5, 0), b)
