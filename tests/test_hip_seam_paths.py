"""Every form of the step-seam kernel (csrc/conv_seam.hpp) that a plan reaches: seam on bit-equal to seam off, and against
the float64 oracle.

tests/fullchip_census.py (a manual, host-only tool) walks dim 32 / 64 / 128, horizon 8 / 16 / 32, transition_dim 2 .. 16,
nets of one to four levels, the option "cc" on and off and every batch 1 .. 2048, asks HipEngine.seam_plan
(dad_debug_seam_plan) for each, and picks by greedy set cover the cases frozen below as CASES: all 5 instantiations
("seam", dim, tile0) and
  ("form", dim, tile0, H, units)   the epilogue's ownership and reduction tree (lpp, width, the rows_sum step, the
                                   two-half add) depend on (dim, H, tile): 15 forms, each with one and two 8-channel units
  ("td", dim, td)                  td in 2, 8, 9, 15, 16: the narrowest, the unit boundary, the widest; a thread of the
                                   posterior owns 4 / 2 / 1 outputs at dim 32 / 64 / 128 and skips those >= td
  ("last", H, tile0, n)            samples in the last tile, 1 .. 32 / H
  ("buffers", dim, relation)       final_act is the very buffer the conv ("dst") or the ride ("rdst") writes
  ("levels", dim, n)               one to four levels: where the activation allocator hands out ids differently
BOUNDARIES are the refusals that depend on the batch ("small-batch kernels", "tile"), and the tile-0 / tile-1 switch, at
their boundary (host test only: a refused plan launches nothing of the family).  The other refusals do not depend on the
batch — option off, split-f16 arithmetic, forced tile, projection, zero-padded net, horizon, transition_dim, dim, first conv,
no riding residual conv hold or fail for an architecture and its options at every batch, so the census space (which varies
the batch) has no boundary for them: tests/test_hip_seam.py::test_report_says_taken_under_the_rule_and_names_every_refusal
asserts each by name and that lifting the one condition gives "taken"; tests/sanitize/seam_check.cpp sweeps them against a
restatement of the rule.  "LDS" and "buffers" are met by no architecture the engine accepts (seam_check.cpp holds the
buffer condition on hand-made plans).

Host (no device): matrix + NOT_REACHED are the library's list, disjoint; the demanded keys are all covered or listed in
UNREACHED with the reason; every case's keys and every boundary hold on today's planner.

GPU, per case: the keys on the plan the engine itself reports, then x after sample_loop with the seam on BIT-EQUAL to x
with it off over n_steps x noise (injected, Philox) x condition (none, shared, per row) x predict_epsilon x
clip_denoised.  The first case of every (dim, tile0, H) form (FULL) runs the whole product of tests/test_hip_seam.py; the
others a pairwise cover of it (_pruned: every pair of option values meets at least once; n_steps 2 and 5, both noise
modes, and both predict_epsilon values are in it).  Once per form the seam-on loop of 5 truncated steps with injected
noise and a shared condition is compared with oracle.sample_loop in float64 on fullchip_census.oracle_subset (whole first,
interior and last tiles, the sample in front of the last tile) at TOL_LOOP; once per instantiation graph replay equals
eager.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import fullchip_census as census
from tests.test_hip_parity import TOL_LOOP, dev  # noqa: F401  (dev: fixture)
from tests.util import as_torch

T = 20
ROW_OFFSET = 2 ** 27 + 3
# seam: 1170 architectures x 2048 batches x cc on / off, 1015 distinct key sets, 5 of 5 instantiations, 77 features
# (id, transition_dim, dim, mults, horizon, batch, cc, the keys the case exists for)
CASES = [
    ('d32_m1_H8_td2_B1_cc0', 2, 32, (1,), 8, 1, 0,
     [('buffers', 32, 'dst'), ('form', 32, 1, 8, 1), ('last', 8, 1, 1), ('levels', 32, 1), ('seam', 32, 1), ('td', 32, 2)]),
    ('d64_m1_H8_td2_B2_cc0', 2, 64, (1,), 8, 2, 0,
     [('buffers', 64, 'dst'), ('form', 64, 1, 8, 1), ('last', 8, 1, 2), ('levels', 64, 1), ('seam', 64, 1), ('td', 64, 2)]),
    ('d128_m1_H8_td2_B3_cc0', 2, 128, (1,), 8, 3, 0,
     [('buffers', 128, 'dst'), ('form', 128, 1, 8, 1), ('last', 8, 1, 3), ('levels', 128, 1), ('seam', 128, 1), ('td', 128, 2)]),
    ('d32_m112_H16_td8_B1_cc0', 8, 32, (1, 1, 2), 16, 1, 0,
     [('buffers', 32, 'rdst'), ('form', 32, 1, 16, 1), ('last', 16, 1, 1), ('levels', 32, 3), ('td', 32, 8)]),
    ('d64_m112_H16_td8_B2_cc0', 8, 64, (1, 1, 2), 16, 2, 0,
     [('buffers', 64, 'rdst'), ('form', 64, 1, 16, 1), ('last', 16, 1, 2), ('levels', 64, 3), ('td', 64, 8)]),
    ('d32_m11_H32_td9_B1_cc0', 9, 32, (1, 1), 32, 1, 0,
     [('form', 32, 1, 32, 2), ('last', 32, 1, 1), ('levels', 32, 2), ('td', 32, 9)]),
    ('d64_m11_H8_td9_B4_cc0', 9, 64, (1, 1), 8, 4, 0,
     [('form', 64, 1, 8, 2), ('last', 8, 1, 4), ('levels', 64, 2), ('td', 64, 9)]),
    ('d128_m112_H16_td8_B1_cc0', 8, 128, (1, 1, 2), 16, 1, 0,
     [('buffers', 128, 'rdst'), ('form', 128, 1, 16, 1), ('levels', 128, 3), ('td', 128, 8)]),
    ('d128_m11_H32_td9_B223_cc1', 9, 128, (1, 1), 32, 223, 1,
     [('form', 128, 0, 32, 2), ('last', 32, 0, 1), ('levels', 128, 2), ('seam', 128, 0), ('td', 128, 9)]),
    ('d64_m1224_H32_td15_B1_cc0', 15, 64, (1, 2, 2, 4), 32, 1, 0,
     [('form', 64, 1, 32, 2), ('levels', 64, 4), ('td', 64, 15)]),
    ('d32_m1_H8_td15_B1_cc0', 15, 32, (1,), 8, 1, 0,
     [('form', 32, 1, 8, 2), ('td', 32, 15)]),
    ('d32_m1_H16_td16_B1_cc0', 16, 32, (1,), 16, 1, 0,
     [('form', 32, 1, 16, 2), ('td', 32, 16)]),
    ('d64_m1_H16_td16_B1_cc0', 16, 64, (1,), 16, 1, 0,
     [('form', 64, 1, 16, 2), ('td', 64, 16)]),
    ('d32_m1224_H32_td2_B1_cc0', 2, 32, (1, 2, 2, 4), 32, 1, 0,
     [('form', 32, 1, 32, 1), ('levels', 32, 4)]),
    ('d128_m1_H8_td15_B1_cc0', 15, 128, (1,), 8, 1, 0,
     [('form', 128, 1, 8, 2), ('td', 128, 15)]),
    ('d128_m1_H16_td16_B1_cc0', 16, 128, (1,), 16, 1, 0,
     [('form', 128, 1, 16, 2), ('td', 128, 16)]),
    ('d64_m1_H16_td2_B893_cc1', 2, 64, (1,), 16, 893, 1,
     [('form', 64, 0, 16, 1), ('last', 16, 0, 1), ('seam', 64, 0)]),
    ('d128_m1_H16_td2_B446_cc1', 2, 128, (1,), 16, 446, 1,
     [('form', 128, 0, 16, 1), ('last', 16, 0, 2)]),
    ('d128_m1224_H32_td2_B1_cc0', 2, 128, (1, 2, 2, 4), 32, 1, 0,
     [('form', 128, 1, 32, 1), ('levels', 128, 4)]),
    ('d64_m1_H32_td2_B1_cc0', 2, 64, (1,), 32, 1, 0,
     [('form', 64, 1, 32, 1)]),
    ('d128_m1_H32_td9_B1_cc0', 9, 128, (1,), 32, 1, 0,
     [('form', 128, 1, 32, 2)]),
    ('d128_m1_H8_td2_B889_cc1', 2, 128, (1,), 8, 889, 1,
     [('form', 128, 0, 8, 1), ('last', 8, 0, 1)]),
    ('d128_m1_H8_td9_B890_cc1', 9, 128, (1,), 8, 890, 1,
     [('form', 128, 0, 8, 2), ('last', 8, 0, 2)]),
    ('d128_m1_H32_td2_B223_cc1', 2, 128, (1,), 32, 223, 1,
     [('form', 128, 0, 32, 1)]),
    ('d64_m1_H32_td2_B447_cc1', 2, 64, (1,), 32, 447, 1,
     [('form', 64, 0, 32, 1)]),
    ('d64_m1_H32_td9_B447_cc1', 9, 64, (1,), 32, 447, 1,
     [('form', 64, 0, 32, 2)]),
    ('d128_m1_H16_td9_B445_cc1', 9, 128, (1,), 16, 445, 1,
     [('form', 128, 0, 16, 2)]),
    ('d64_m1_H8_td2_B1787_cc1', 2, 64, (1,), 8, 1787, 1,
     [('form', 64, 0, 8, 1), ('last', 8, 0, 3)]),
    ('d64_m1_H8_td9_B1788_cc1', 9, 64, (1,), 8, 1788, 1,
     [('form', 64, 0, 8, 2), ('last', 8, 0, 4)]),
    ('d64_m1_H16_td9_B893_cc1', 9, 64, (1,), 16, 893, 1,
     [('form', 64, 0, 16, 2)]),
]
NOT_REACHED = []
# (architecture (td, dim, mults, H), cc, last batch in the first state, first batch in the second, (reason, tile) before, after)
BOUNDARIES = [
    ((6, 32, (1,), 32), 1, 16, 17, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 64, (1,), 32), 1, 16, 17, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 128, (1,), 32), 1, 16, 17, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 32, (1,), 16), 1, 32, 33, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 64, (1,), 16), 1, 32, 33, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 128, (1,), 16), 1, 32, 33, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 32, (1,), 8), 1, 64, 65, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 64, (1,), 8), 1, 64, 65, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 128, (1,), 8), 1, 64, 65, ('small-batch kernels', -1), ('taken', 0)),
    ((6, 128, (1,), 32), 1, 222, 223, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 32), 0, 222, 223, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 16), 1, 444, 445, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 16), 0, 444, 445, ('taken', 0), ('taken', 1)),
    ((6, 64, (1,), 32), 1, 446, 447, ('taken', 0), ('taken', 1)),
    ((6, 64, (1,), 32), 0, 446, 447, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 8), 1, 888, 889, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 8), 0, 888, 889, ('taken', 0), ('taken', 1)),
    ((6, 64, (1,), 16), 1, 892, 893, ('taken', 0), ('taken', 1)),
    ((6, 64, (1,), 16), 0, 892, 893, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 32), 1, 1022, 1023, ('taken', 1), ('tile', -1)),
    ((6, 128, (1,), 32), 0, 1022, 1023, ('taken', 1), ('tile', -1)),
    ((6, 64, (1,), 8), 1, 1784, 1785, ('taken', 0), ('taken', 1)),
    ((6, 64, (1,), 8), 0, 1784, 1785, ('taken', 0), ('taken', 1)),
    ((6, 128, (1,), 16), 1, 2044, 2045, ('taken', 1), ('tile', -1)),
    ((6, 128, (1,), 16), 0, 2044, 2045, ('taken', 1), ('tile', -1)),
]
FORMS = [(32, 1, H) for H in (8, 16, 32)] + [(dim, t0, H) for dim in (64, 128) for t0 in (1, 0) for H in (8, 16, 32)]
# what the matrix must cover
DEMANDED = ([("seam", d, t0) for d, t0 in ((32, 1), (64, 1), (64, 0), (128, 1), (128, 0))] +
            [("form", d, t0, H, u) for d, t0, H in FORMS for u in (1, 2)] + [("td", d, td) for d in (32, 64, 128) for td in census.SEAM_TDS] +
            [("last", H, t0, n) for H in (8, 16, 32) for t0 in (1, 0) for n in range(1, 32 // H + 1)] +
            [("levels", d, n) for d in (32, 64, 128) for n in (1, 2, 3, 4)] +
            [("buffers", d, r) for d in (32, 64, 128) for r in ("dst", "rdst", "apart")])
_APART = ("the activation allocator hands final_conv[0] the first free level-0 buffer, and by then the first block's two outputs are free: on "
          "every net of the census space final_act is the buffer the first conv or its ride writes, never a third one")
UNREACHED = {("buffers", d, "apart"): _APART for d in (32, 64, 128)}


def _form(case):
    return next(k[1:4] for k in case[-1] if k[0] == "form")


# the first case of every form runs the whole option product and meets the oracle; the first of every instantiation replays a graph
FULL = {}
for _c in CASES:
    FULL.setdefault(_form(_c), _c[0])
GRAPH = {}
for _c in CASES:
    GRAPH.setdefault(_form(_c)[:2], _c[0])

N_STEPS, NOISE, COND, PE, CLIP = (1, 2, 5), ("injected", "philox"), ("none", "shared", "rows"), (1, 0), (1, 0)


def _pairs(row):
    return {(a, row[a], b, row[b]) for a, b in itertools.combinations(range(5), 2)}


def _pruned(seed):
    """A pairwise cover of N_STEPS x NOISE x COND x PE x CLIP: every pair of values of any two options meets in some row
    (so every value of every option is in it: n_steps 2 and 5, both noise modes, both predict_epsilon values).  Greedy
    and deterministic; `seed` rotates the order the product is searched in, so that the cases do not all run the same
    rows."""
    product = list(itertools.product(N_STEPS, NOISE, COND, PE, CLIP))
    at = (seed * 7) % len(product)
    product = product[at:] + product[:at]
    need = set().union(*(_pairs(r) for r in product))
    rows = []
    while need:
        best = max(product, key=lambda r: len(_pairs(r) & need))
        rows.append(best)
        need -= _pairs(best)
    return rows


def _covers_pairs(rows):
    product = itertools.product(N_STEPS, NOISE, COND, PE, CLIP)
    return set().union(*(_pairs(r) for r in product)) == set().union(*(_pairs(r) for r in rows))


def _host(case, **options):
    _, td, dim, mults, H, B, cc, _ = case
    eng = census.host_engine(td, dim, mults, H, 5, "fp32")
    census.set_all(eng, dict({"cc": cc}, **options))
    return eng


# ------------------------------------------------------------------------------------------------ host
def test_matrix_and_not_reached_are_the_registered_instantiations():
    from dynamics_aware_diffusion_amd._engine import fullchip_kernels
    _, registered = fullchip_kernels()
    matrix = {k for c in CASES for k in c[-1] if k[0] == "seam"}
    assert len(registered) == 5
    assert matrix | set(NOT_REACHED) == registered and not matrix & set(NOT_REACHED)
    assert not NOT_REACHED, "every instantiation is reached"


def test_every_demanded_key_is_reached_or_explained():
    covered = {k for c in CASES for k in c[-1]}
    assert covered <= set(DEMANDED), sorted(covered - set(DEMANDED))
    assert not covered & set(UNREACHED)
    assert covered | set(UNREACHED) == set(DEMANDED), sorted(set(DEMANDED) - covered - set(UNREACHED))
    assert len(FORMS) == 15 and set(FULL) == set(FORMS) and len(GRAPH) == 5
    # what the issue names one by one
    for k in [("last", 8, 1, 2), ("last", 8, 1, 3), ("last", 8, 0, 2), ("last", 8, 0, 3), ("levels", 32, 3), ("levels", 32, 4), ("levels", 128, 3),
              ("levels", 128, 4)] + [("td", d, td) for d in (32, 64, 128) for td in (2, 8, 9, 15, 16)]:
        assert k in covered, k
    for seed in range(len(CASES)):
        rows = _pruned(seed)
        assert _covers_pairs(rows) and {r[0] for r in rows} >= {2, 5} and {r[1] for r in rows} == set(NOISE) and {r[3] for r in rows} == set(PE), seed


def test_case_keys_and_boundaries_hold_on_todays_planner():
    for case in CASES:
        name, td, dim, mults, H, B, cc, keys = case
        q = _host(case).seam_plan(B, detail=True)
        assert q["taken"] and set(keys) <= census.seam_keys(q, dim, td, len(mults)), (name, q)
        assert q["grid"] == (B * H + 31) // 32 and q["spt"] == 32 // H and (q["grid"] - 1) * q["spt"] + q["last"] == B
        assert _host(case, step_seam=0).seam_plan(B, detail=True)["reason"] == "option off"
    for arch, cc, b0, b1, before, after in BOUNDARIES:
        eng = census.host_engine(*arch, 5, "fp32")
        census.set_all(eng, {"cc": cc})
        for B, (reason, tile) in ((b0, before), (b1, after)):
            q = eng.seam_plan(B, detail=True)
            assert (q["reason"], q["tile"]) == (reason, tile), (arch, cc, B, q)
    # no net of the cases, at any batch up to 64, keeps final_act apart from both buffers (UNREACHED)
    for case in CASES:
        eng = _host(case)
        assert {eng.seam_plan(B, detail=True)["buffers"] for B in (1, 2, 3, 5, 17, 33, 64)} <= {"dst", "rdst", None}, case[0]


# ------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _inputs(name):
    """Weights, start, injected noise and conditions of a case; nobody writes into them."""
    from dynamics_aware_diffusion_amd.utils import synth
    _, td, dim, mults, H, B, _, _ = next(c for c in CASES if c[0] == name)
    state = synth.synth_unet_state(td, dim, mults, seed=67, affine_jitter=0.3)
    noise = torch.from_numpy(synth.normal_like(41, "seamp.noise." + name, (6, B, H, td)))
    cond = torch.from_numpy(synth.uniform(41, "seamp.cond." + name, (B, td), 0.9))
    return {"state": state, "noise": noise, "cond": cond}


def _engine(case, dev, **kw):
    from tests.test_hip_long_horizon import _diffusion
    name, td, dim, mults, H, B, cc, keys = case
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, _inputs(name)["state"], dev, **kw)
    eng = diff._engine(dev)
    eng.debug_set_option("cc", cc)
    q = eng.seam_plan(B, detail=True)
    assert q["taken"] and set(keys) <= census.seam_keys(q, dim, td, len(mults)), (name, q)
    return diff, eng


def _loop(eng, inp, dev, n_steps, noise_mode, cond_mode, **kw):
    x = inp["noise"][0].to(dev).clone()
    cond = {"none": None, "shared": inp["cond"][:1], "rows": inp["cond"]}[cond_mode]
    if cond is not None:
        cond = cond.to(dev).contiguous()
        x[:, 0] = cond
    if noise_mode == "injected":
        eng.sample_loop(x, n_steps, noise_stack=inp["noise"][1:1 + n_steps].to(dev).contiguous(), cond0=cond, **kw)
    else:
        eng.sample_loop(x, n_steps, seed=0x123456789ABCDEF, row_offset=ROW_OFFSET, cond0=cond, **kw)
    torch.cuda.synchronize()
    return x.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_seam_case_on_is_bit_equal_to_off(case, dev):
    name, td, dim, mults, H, B, cc, keys = case
    inp = _inputs(name)
    full = FULL[_form(case)] == name
    rows = list(itertools.product(N_STEPS, NOISE, COND, PE, CLIP)) if full else _pruned(CASES.index(case))
    worst, engines = 0.0, {}
    for n_steps, noise_mode, cond_mode, pe, clip in rows:
        if (pe, clip) not in engines:
            engines[(pe, clip)] = _engine(case, dev, predict_epsilon=bool(pe), clip_denoised=bool(clip))
        diff, eng = engines[(pe, clip)]
        got = {}
        try:
            for on in (1, 0):
                eng.debug_set_option("step_seam", on)
                assert eng.seam_plan(B, detail=True)["taken"] == bool(on)
                got[on] = _loop(eng, inp, dev, n_steps, noise_mode, cond_mode)
        finally:
            eng.debug_set_option("step_seam", 1)
        assert diff.model._engine is eng
        assert torch.isfinite(got[1]).all()
        d = float((got[1] - got[0]).abs().max())
        worst = max(worst, d)
        assert torch.equal(got[1], got[0]), (name, pe, clip, n_steps, noise_mode, cond_mode, d)
    print(f"\n{name}: {len(rows)} loops, max |seam on - seam off| = {worst:.1e}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if FULL[_form(c)] == c[0]], ids=lambda c: c[0])
def test_seam_form_loop_vs_float64(case, dev):
    """The last 5 reverse steps of the T = 20 schedule (a truncated loop, as the loop cases of tests/test_hip_parity.py) with
    injected noise and an inpainted first row, against the float64 oracle on the sample subset; a second call gives the
    same bits."""
    from oracle import denoiser as orc
    name, td, dim, mults, H, B, cc, keys = case
    steps = 5
    inp = _inputs(name)
    sub = census.oracle_subset(B, 32 // H)
    cond = inp["cond"][:1]
    w64 = orc.cast_weights(as_torch(inp["state"]), torch.float64)
    s64 = {k: v.double() for k, v in orc.schedule_buffers("cosine", T).items()}
    want = orc.sample_loop(w64, s64, inp["noise"][:, sub].double(), steps, {0: cond.double()})
    _, eng = _engine(case, dev)
    got = _loop(eng, inp, dev, steps, "injected", "shared")
    err = float((got[sub].double() - want).abs().max())
    print(f"\nseam loop {name} T={steps}: on {len(sub)} samples |hip - float64| = {err:.2e}")
    assert np.isfinite(err) and err <= TOL_LOOP
    assert torch.isfinite(got).all()
    assert torch.equal(got, _loop(eng, inp, dev, steps, "injected", "shared")), "a second call gives other bits"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if GRAPH[_form(c)[:2]] == c[0]], ids=lambda c: c[0])
def test_seam_instantiation_graph_replay_equals_eager(case, dev):
    inp = _inputs(case[0])
    _, eng = _engine(case, dev)
    for noise_mode in NOISE:
        first = _loop(eng, inp, dev, 5, noise_mode, "shared")
        graph = _loop(eng, inp, dev, 5, noise_mode, "shared", use_graph=True)
        assert torch.equal(first, graph), "graph replay differs from eager"
        assert torch.equal(graph, _loop(eng, inp, dev, 5, noise_mode, "shared", use_graph=True)), "a second replay gives other bits"
