"""CPU tests (`-m "not gpu"`): the C-ABI library loads and exports what include/dad.h declares,
and the host-side mirror of the reference API (schedules, state_dict schema, projector
builder, planner glue, sharding) behaves like the reference.  No compute call needs a GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.util import GOLDEN, golden, max_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------- ABI
def _header_functions():
    text = open(os.path.join(ROOT, "include", "dad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dad_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from dynamics_aware_diffusion_amd import _engine
    declared = _header_functions()
    assert len(declared) >= 15
    assert sorted(_engine.ABI) == declared, "ctypes table and include/dad.h disagree"
    lib = _engine.load_library()                    # raises if the .so is missing
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.dad_version()


def test_abi_rejects_bad_arguments_without_a_gpu():
    """Argument validation happens before any HIP call, so it is checkable on CPU."""
    import ctypes as C
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    cfg = _engine.DadCfg()
    cfg.transition_dim, cfg.dim, cfg.time_dim, cfg.n_levels = 6, 32, 32, 3
    for i, ch in enumerate((32, 64, 128)):
        cfg.channels[i] = ch
    cfg.kernel_size, cfg.horizon, cfg.n_timesteps = 5, 32, 20
    cfg.predict_epsilon = cfg.clip_denoised = 1
    h = C.c_void_p()
    assert lib.dad_model_create(C.byref(cfg), C.byref(h)) == 0
    n = C.c_size_t()
    assert lib.dad_workspace_bytes(h, 4, C.byref(n)) == 0 and n.value > 0
    # unknown key / wrong shape
    buf = (C.c_float * 8)()
    shape = (C.c_int64 * 1)(8)
    assert lib.dad_model_load_weight(h, b"no.such.key", buf, shape, 1) == -3
    assert b"no.such.key" in lib.dad_last_error()
    assert lib.dad_model_load_weight(h, b"final_conv.1.bias", buf, shape, 1) == -3   # 6 expected
    # step before finalize
    assert lib.dad_unet_forward(h, None, 0, None, 1, None, 0, None) == -2
    # conv arithmetic: the two known modes, anything else refused
    assert lib.dad_model_set_precision(h, 1) == 0 and lib.dad_model_set_precision(h, 0) == 0
    assert lib.dad_model_set_precision(h, 7) == -1 and b"precision" in lib.dad_last_error()
    assert lib.dad_model_set_precision(None, 0) == -1
    lib.dad_model_destroy(h)
    # unsupported architectures are refused with a message, not a crash
    for ks in (4, 9, 1):                                # 3, 5 and 7 exist
        cfg.kernel_size = ks
        assert lib.dad_model_create(C.byref(cfg), C.byref(h)) == -1
    cfg.kernel_size, cfg.horizon = 5, 8                 # 8 / 2^2 = 2 < 4
    assert lib.dad_model_create(C.byref(cfg), C.byref(h)) == -1
    cfg.horizon = 32
    cfg.channels[1] = 48                                # not a multiple of 32
    assert lib.dad_model_create(C.byref(cfg), C.byref(h)) == -1


def test_zero_padded_groups_keep_every_real_weight():
    """utils/padding.py: a --dim 48 net (GroupNorm groups of 6 / 12 channels) becomes a 64 / 128-channel net whose
    extra channels are zero; every real entry sits where channel_index says, and the padded shapes are what the
    library expects for the padded widths (dad_model_load_weight checks them against its own plan)."""
    import ctypes as C
    from dynamics_aware_diffusion_amd import _engine
    from dynamics_aware_diffusion_amd.utils import padding, synth
    assert [padding.padded_width(c) for c in (8, 24, 32, 48, 64, 96, 120, 128, 2048)] == [32, 32, 32, 64, 64, 128, 128, 128, 2048]
    with pytest.raises(ValueError):
        padding.padded_width(44)
    idx = padding.channel_index(48)
    assert idx.tolist()[:7] == [0, 1, 2, 3, 4, 5, 8] and int(idx[-1]) == 7 * 8 + 5
    td, dim, mults = 6, 48, (1, 2)
    state = {k: torch.from_numpy(v) for k, v in synth.synth_unet_state(td, dim, mults, seed=2, affine_jitter=0.2).items()}
    padded, pdim, widths = padding.pad_unet_state(state, td, dim, mults)
    assert pdim == 64 and widths == [64, 128] and set(padded) == set(state)
    i48, i96 = padding.channel_index(48), padding.channel_index(96)
    w = padded["downs.1.0.blocks.0.block.0.weight"]                      # Conv1d(48 -> 96, k5)
    assert tuple(w.shape) == (128, 64, 5)
    assert torch.equal(w[i96][:, i48], state["downs.1.0.blocks.0.block.0.weight"])
    assert int(w.count_nonzero()) == int(state["downs.1.0.blocks.0.block.0.weight"].count_nonzero())
    u = padded["ups.0.0.blocks.0.block.0.weight"]                        # Conv1d(cat[96 | 96] -> 48)
    assert tuple(u.shape) == (64, 256, 5)
    assert torch.equal(u[i48][:, torch.cat([i96, 128 + i96])], state["ups.0.0.blocks.0.block.0.weight"])
    t = padded["ups.0.2.conv.weight"]                                    # ConvTranspose1d(48, 48): (in, out, k)
    assert torch.equal(t[i48][:, i48], state["ups.0.2.conv.weight"])
    g = padded["final_conv.0.block.1.weight"]
    assert torch.equal(g[i48], state["final_conv.0.block.1.weight"]) and int(g.count_nonzero()) == 48
    assert tuple(padded["final_conv.1.weight"].shape) == (td, 64, 1) and tuple(padded["time_mlp.1.weight"].shape) == (4 * 48, 64)
    # all tensors with ONE scatter (what training and the device-side refresh use): the same padded tensors, and autograd
    # carries the gradient of a padded tensor back onto the real entries only
    keys = list(state)
    plan, _, _ = padding.padding_plan(keys, td, dim, mults)
    leaves = [state[k].clone().requires_grad_(True) for k in keys]
    flat = padding.FlatPadding(keys, [tuple(state[k].shape) for k in keys], plan)
    with torch.enable_grad():
        wide = flat.pad(leaves)
        assert all(torch.equal(a.detach(), padded[k]) for a, k in zip(wide, keys))
        sum((a * torch.arange(a.numel(), dtype=torch.float32).view(a.shape)).sum() for a in wide).backward()
    for leaf, k in zip(leaves, keys):
        want = padding.unpad_tensor(torch.arange(padded[k].numel(), dtype=torch.float32).view(padded[k].shape), plan[k])
        assert torch.equal(leaf.grad, want), k
    # ... and back: one gather of the real entries out of a flat padded vector laid out at given offsets (the engine's
    # gradient buffer), tensors 16-byte aligned
    offs, at = [], 8
    for n in flat.sizes:
        offs.append(at)
        at += (n + 3) // 4 * 4 + 4
    spaced = padding.FlatPadding(keys, [tuple(state[k].shape) for k in keys], plan, offs, at)
    back = spaced.gather(spaced.pad_flat([state[k] for k in keys]))
    assert all(torch.equal(b, state[k]) for b, k in zip(back, keys)) and all(o % 4 == 0 for o in flat.offsets)
    # the library's own expectations for the padded widths
    lib = _engine.load_library()
    cfg = _engine.DadCfg()
    cfg.transition_dim, cfg.dim, cfg.time_dim, cfg.n_levels = td, 64, 48, 2
    cfg.channels[0], cfg.channels[1] = 64, 128
    cfg.kernel_size, cfg.horizon, cfg.n_timesteps = 5, 32, 10
    cfg.predict_epsilon = cfg.clip_denoised = 1
    h = C.c_void_p()
    assert lib.dad_model_create(C.byref(cfg), C.byref(h)) == 0
    real = (C.c_int32 * 2)(48, 96)
    assert lib.dad_model_set_group_channels(h, real, 2) == 0
    for key, v in padded.items():
        v = v.contiguous()
        shape = (C.c_int64 * v.dim())(*v.shape)
        assert lib.dad_model_load_weight(h, key.encode(), v.data_ptr(), shape, v.dim()) == 0, (key, lib.dad_last_error())
    assert lib.dad_model_set_training(h, 1) == 0, lib.dad_last_error()       # padded widths train (the channel map stays in Python)
    bad = (C.c_int32 * 2)(44, 96)
    assert lib.dad_model_set_group_channels(h, bad, 2) == -1
    assert lib.dad_model_set_group_channels(h, real, 3) == -1
    lib.dad_model_destroy(h)


def test_horizon_padding_entry_point():
    """dad_model_set_horizon: the padded (power-of-two) horizon lives in dad_cfg, the real one must be a multiple of
    2^(levels-1) below it; such models refuse training."""
    import ctypes as C
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    cfg = _pointmaze_cfg()                      # 3 levels, horizon 32
    h = C.c_void_p()
    assert lib.dad_model_create(C.byref(cfg), C.byref(h)) == 0
    for bad in (0, 2, 22, 36, -4):              # below 2^(levels-1), not a multiple of 4, above the padded horizon
        assert lib.dad_model_set_horizon(h, bad) == -1, bad
    assert lib.dad_model_set_horizon(h, 24) == 0
    assert lib.dad_model_set_training(h, 1) == 0          # (a zero-padded horizon trains; zero-padded widths do not)
    assert lib.dad_model_set_horizon(h, 32) == 0          # back to the unpadded model
    assert lib.dad_model_set_training(h, 1) == 0
    lib.dad_model_destroy(h)
    with pytest.raises(ValueError, match="halved"):
        _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=22, n_timesteps=10)


def test_planner_and_kernel_registry_agree():
    """The planner refuses launches no kernel was compiled for by one predicate per kernel family (csrc/host_plan.hpp
    kFamilies: kernel_registered and its like — what the sanitizer harness checks launch plans against), and the
    library's kernel registry is generated from those predicates: for each of the six families the table must hold an
    entry wherever the predicate is true over its whole domain and nothing else (round 3: a 3-tap conv under the
    split-f16 arithmetic was planned onto a kernel that does not exist).  The registry's own list of each family has
    the family's count of distinct keys."""
    import ctypes as C
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    assert lib.dad_debug_kernel_table_consistent() == 1, lib.dad_last_error()
    counts = {family: len(_engine.kernel_list(family)) for family in _engine.KERNEL_FAMILIES}
    assert counts == {"gemm": 335, "cc": 18, "ccw": 20, "halo8": 4, "seam": 5, "wgrad": 40}
    need = C.c_int32()
    assert lib.dad_debug_kernel_list(len(_engine.KERNEL_FAMILIES), None, 0, C.byref(need)) == -1       # no such family


def test_report_layouts_are_the_ones_every_reader_was_written_against():
    """The plan reports are the instrument the censuses and the path tests read plans through, and the binding decodes
    them by the field lists the library exports (dad_debug_report_layout), so a field that moved would move silently.
    tests/golden/report_layouts.json holds every DAD_{FP,BP,BS,OP,H8,SEAM,PP,OS}_* constant as include/dad.h defined them
    by hand before the layouts were stated as lists: each is rebuilt from the export — a field's offset is the sum of the
    spans before it, a section's length constant the sum of all its spans — and must be there with that value."""
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    assert lib.dad_debug_report_layout(-1, 0) is None and lib.dad_debug_report_layout(0, -1) is None
    assert lib.dad_debug_report_layout(1000, 0) is None and lib.dad_debug_report_layout(0, 1000) is None
    layouts = _engine.report_layouts()
    rebuilt = {}
    for length, fields in layouts.items():
        names = [name for _, name, _ in fields if name != "_"]
        assert len(names) == len(set(names)), f"{length}: a field name twice"
        at = 0
        for constant, _, span in fields:
            assert span >= 1 and rebuilt.setdefault(constant, at) == at, (length, constant)
            at += span
        assert rebuilt.setdefault(length, at) == at, length
    with open(os.path.join(GOLDEN, "report_layouts.json")) as fh:
        pinned = json.load(fh)
    assert len(pinned) == 213
    assert {k: rebuilt.get(k) for k in pinned} == pinned
    spans = {c: s for fields in layouts.values() for c, n, s in fields if s != 1 and n != "_"}
    assert spans == {"DAD_BP_TILE": 4, "DAD_BP_TAPS_TILE": 20, "DAD_BP_FWD": 20, "DAD_BP_DGRAD": 20}


def test_every_report_says_the_record_length_its_layout_states():
    """The header field ``record_ints`` of each report with records, read from real reports (engines without weights or
    a device), is the length of the record section the export gives: of every kind of record the report holds."""
    from dynamics_aware_diffusion_amd import _engine
    length = lambda section: _engine._fields(section)[1]
    eng = _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=10, training=True)
    lib, h = eng.lib, eng._h

    def record_ints(header, fn, *args):
        return _engine._decode(header, _engine._fetch(fn, *args))["record_ints"]

    assert record_ints("DAD_BP_HEADER", lib.dad_debug_backward_plan, h, 4) == length("DAD_BP_REC_INTS")
    steps = record_ints("DAD_BS_HEADER", lib.dad_debug_backward_steps, h, 4)
    kinds = _engine._names("DAD_BS_KINDS")
    assert len(kinds) == 6 and {length(f"DAD_BS_{kind.upper()}_INTS") for kind in kinds} == {steps} == {length("DAD_BS_REC_INTS")}
    assert record_ints("DAD_OP_HEADER", lib.dad_debug_objective_plan, h, 4) == length("DAD_OP_REC_INTS")
    assert eng.forward_plan(1)["small"] and not eng.forward_plan(256)["small"]
    assert record_ints("DAD_FP_HEADER", lib.dad_debug_forward_plan, h, 1, 0) == length("DAD_FP_CC_INTS")
    assert record_ints("DAD_FP_HEADER", lib.dad_debug_forward_plan, h, 256, 0) == length("DAD_FP_REC_INTS")
    assert eng.halo8_plan(1024), "no conv_halo8_f32 launch: the record length below would be read from an empty report"
    assert record_ints("DAD_H8_HEADER", lib.dad_debug_halo8_plan, h, 1024, 0) == length("DAD_H8_INTS")
    import ctypes as C
    assert record_ints("DAD_OS_HEADER", lib.dad_debug_optim_plan, (C.c_int64 * 2)(5000, 7), 2) == length("DAD_OS_REC_INTS")


def _pointmaze_cfg():
    from dynamics_aware_diffusion_amd import _engine
    cfg = _engine.DadCfg()
    cfg.transition_dim, cfg.dim, cfg.time_dim, cfg.n_levels = 6, 128, 128, 3
    for i, ch in enumerate((128, 256, 512)):
        cfg.channels[i] = ch
    cfg.kernel_size, cfg.horizon, cfg.n_timesteps = 5, 32, 100
    cfg.predict_epsilon = cfg.clip_denoised = 1
    return cfg


def test_debug_hooks_are_per_model():
    """no global state behind the ABI.  Tile / split-K / fusion hooks set on one
    model leave another model in the same process untouched (checked through the workspace size,
    which depends on the tile choice and on grid-level split-K — no GPU needed)."""
    import ctypes as C
    from dynamics_aware_diffusion_amd import _engine
    lib = _engine.load_library()
    cfg = _pointmaze_cfg()
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.dad_model_create(C.byref(cfg), C.byref(a)) == 0
    assert lib.dad_model_create(C.byref(cfg), C.byref(b)) == 0

    def ws(h, batch):
        n = C.c_size_t()
        assert lib.dad_workspace_bytes(h, batch, C.byref(n)) == 0
        return n.value

    # batch 32 is beyond the small-batch kernels: its scratch is the grid split-K slabs
    base = ws(b, 32)
    assert ws(a, 32) == base
    assert lib.dad_debug_set_tile(a, 99) == 0              # heuristic tiles, grid split-K off
    assert ws(a, 32) < base                                # no split-K slabs any more
    assert ws(b, 32) == base                               # the other model did not notice
    assert lib.dad_debug_set_option(a, b"split_target", 64) == 0
    assert lib.dad_debug_set_option(a, b"no_such_option", 1) == -1
    assert b"no_such_option" in lib.dad_last_error()
    assert lib.dad_debug_set_option(a, b"chain", 1) == -1                 # the level-0 chain kernel was removed
    assert b"unknown option" in lib.dad_last_error()
    assert lib.dad_debug_set_tile(a, -1) == 0
    assert ws(a, 32) < base and ws(b, 32) == base          # split target 64 < 256: smaller slabs
    # the small-batch (consumer-combine) kernels are a per-model switch as well
    one = ws(b, 1)
    assert lib.dad_debug_set_option(a, b"cc", 0) == 0 and lib.dad_debug_set_option(a, b"split_target", 256) == 0
    assert ws(a, 1) != one and ws(b, 1) == one
    assert lib.dad_debug_set_tile(None, 1) == -1
    # table read-back and the time-embedding upload validate before touching the device
    buf = (C.c_float * 16)()
    assert lib.dad_debug_read_table(a, 0, 0, buf, 16, None) == -2          # not finalized
    assert lib.dad_model_load_time_embedding(a, buf, 7, 128) == -1         # wrong shape
    assert lib.dad_debug_mish(None, None, 4, None) == -1
    lib.dad_model_destroy(a)
    lib.dad_model_destroy(b)


def test_host_logic_and_weight_table_under_address_and_ub_sanitizers(tmp_path):
    """the launch planner, the weight table and its packed images (bit for bit
    against explicit packing loops kept in the harness), split-f16 imaging, tile / split-K choice and
    LDS slot-shift search compiled host-only with -fsanitize=address,undefined and run over the
    five architectures plus the fuzz generator's space (tests/sanitize/host_check.cpp).  CPU
    build only — GPU sanitizers are not available on this pool."""
    import shutil
    cxx = shutil.which("amdclang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx) or shutil.which(cxx), "ROCm clang++ not found"
    exe = tmp_path / "host_check"
    src = os.path.join(ROOT, "tests", "sanitize", "host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                            "-Werror", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
                                  UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "host logic ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_device_kernels_use_no_scratch(tmp_path):
    """Register spills are a performance cliff for the hand-written kernels (a spilled staging
    register turned a 75 ms loop into 111 ms in round 2): compile the device side of the library to
    gfx950 assembly and require `private_segment_fixed_size == 0` for every conv-GEMM kernel, the
    pointwise kernels and the common small-batch kernels (the 9..16-slab variants, two launches of a
    PointMaze step, are allowed their 20 bytes; so is the 7-tap direct-B tile of 2048-channel layers)."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = tmp_path / "dad.s"
    src = os.path.join(ROOT, "dynamics_aware_diffusion_amd", "csrc", "dad_lib.hip")
    run = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-S", "--cuda-device-only",
                          "-o", str(asm), src], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    text = asm.read_text()
    kernels = re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, flags=re.S)
    assert len(kernels) > 100
    spilled = {n: int(b) for n, b in kernels if int(b) > 0}
    allowed = {n for n in spilled if "conv_cc" in n and "ELb1ELi" in n and spilled[n] <= 32}   # BIG variants
    # kernel_size=7 on 2048-channel layers (no recipe uses it): the direct-B tile rolls seven taps' fragments
    allowed |= {n for n in spilled if "conv_gemm_f32ILi256ELi32ELi1ELi32ELi7E" in n and spilled[n] <= 96}
    assert set(spilled) == allowed, {n: b for n, b in spilled.items() if n not in allowed}
    assert text.count("v_mfma_f32_32x32x2") > 1000 and text.count("v_mfma_f32_16x16x4") > 50


def test_precision_names_are_validated_before_any_device_call():
    from dynamics_aware_diffusion_amd import _engine
    assert _engine.PRECISIONS == {"fp32": 0, "f16x3": 1}
    with pytest.raises(ValueError, match="precision"):
        _engine.HipEngine(transition_dim=6, dim=32, channels=(32, 64), horizon=32, n_timesteps=10,
                          precision="bf16")


def test_missing_library_fails_loudly(tmp_path, monkeypatch):
    from dynamics_aware_diffusion_amd import _engine
    monkeypatch.setattr(_engine, "_lib", None)
    monkeypatch.setattr(_engine, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _engine.load_library()


# ------------------------------------------------------------------------------ schedules
def test_schedule_buffers_match_reference_bitwise():
    from dynamics_aware_diffusion_amd.models.diffusion import make_schedule
    g = golden("schedules")
    for name, T in cases.SCHEDULE_CASES:
        bufs = make_schedule(name, T)
        assert list(bufs) == [k.split(".", 1)[1] for k in g.files if k.startswith(f"{name}_{T}.")]
        for k, v in bufs.items():
            assert np.array_equal(v.numpy(), g[f"{name}_{T}.{k}"]), (name, T, k)
    with pytest.raises(ValueError, match="Unknown beta schedule"):
        make_schedule("sigmoid", 10)


def test_state_dict_schema_matches_reference():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    want = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))
    for net in ("tiny", "tiny4", "pointmaze"):
        od, ad, td, dim, mults = cases.net_dims(net)
        diff = GaussianDiffusion(TemporalUnet(td, dim=dim, dim_mults=mults), cases.H, od, ad,
                                 n_timesteps=cases.NETS[net][4])
        sd = diff.state_dict()
        ref = dict(want[net]["buffers"], **want[net]["model"])
        assert list(sd) == want[net]["order"], net              # same keys, same order
        for k, v in sd.items():
            assert list(v.shape) == ref[k], (net, k)
    # big nets: shapes only (no allocation)
    from dynamics_aware_diffusion_amd.utils.synth import unet_param_shapes
    for net in ("halfcheetah", "door"):
        od, ad, td, dim, mults = cases.net_dims(net)
        shapes = unet_param_shapes(td, dim, mults, prefix="model.")
        assert {k: list(v) for k, v in shapes.items()} == want[net]["model"]


def test_diffusion_attributes_and_errors():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    unet = TemporalUnet(6, dim=32, dim_mults=(1, 2))
    d = GaussianDiffusion(unet, 32, 4, 2, n_timesteps=50, beta_schedule="linear")
    assert (d.horizon, d.observation_dim, d.action_dim, d.transition_dim) == (32, 4, 2, 6)
    assert d.n_timesteps == 50 and d.betas.shape == (50,) and d.beta_schedule == "linear"
    d.n_timesteps = 10                                   # evaluate.py:352 mutates it
    with pytest.raises(ValueError, match="Unknown loss type"):
        GaussianDiffusion(unet, 32, 4, 2, loss_type="huber")
    with pytest.raises(ValueError, match="Unknown beta schedule"):
        GaussianDiffusion(unet, 32, 4, 2, beta_schedule="exp")
    # closed forms stay plain torch and work on CPU (training-side helpers)
    x0 = torch.randn(3, 32, 6)
    t = torch.tensor([0, 5, 49])
    z = torch.randn_like(x0)
    xt = d.q_sample(x0, t, z)
    assert torch.allclose(d.predict_start_from_noise(xt, t, z), x0, atol=1e-4)
    mean, logvar = d.q_posterior(x0, xt, t)
    assert mean.shape == x0.shape and logvar.shape == (3, 1, 1)
    with pytest.raises(RuntimeError):                    # gather out of range, like the reference
        d.q_sample(x0, torch.tensor([0, 5, 50]), z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # forward-only loss runs on the engine
        d.loss(x0)


# ------------------------------------------------------------------------------ checkpoints
def _synthetic_checkpoint(td, dim, mults, od, ad, T=20, horizon=32, time_dim=None, ema_seed=None, kernel_size=5):
    """The dict the reference's trainer saves (utils/training.py:191-211), synthetic weights."""
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    from dynamics_aware_diffusion_amd.utils import synth

    def state(seed):
        unet = TemporalUnet(td, dim=dim, dim_mults=mults, time_dim=time_dim, kernel_size=kernel_size)
        w = synth.synth_unet_state(td, dim, mults, seed=seed, affine_jitter=0.2, time_dim=time_dim, kernel_size=kernel_size)
        unet.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        return GaussianDiffusion(unet, horizon, od, ad, n_timesteps=T).state_dict(), w

    sd, w = state(5)
    ckpt = {"epoch": 3, "global_step": 1234, "model_state_dict": sd, "optimizer_state_dict": {},
            "config": {"horizon": horizon, "observation_dim": od, "action_dim": ad, "n_timesteps": T,
                       "beta_schedule": "cosine"}}
    w_ema = None
    if ema_seed is not None:
        ckpt["ema_state_dict"], w_ema = state(ema_seed)
    return ckpt, w, w_ema


def test_checkpoint_architecture_is_inferred_from_shapes(tmp_path):
    """SURVEY 8(f) rank 1 / finding F9: per-level widths come from tensor shapes, so (1, 4, 8) and
    other non-power-of-two nets load (the reference's evaluate.py:90-99 guesses from the level
    count); EMA weights can be selected; a wrong or missing key is a clear error."""
    from dynamics_aware_diffusion_amd import infer_architecture, load_checkpoint
    want = json.load(open(os.path.join(GOLDEN, "state_dict_keys.json")))
    for (td, dim, mults, od, ad, tdim) in ((23, 32, (1, 4, 8), 17, 6, None), (8, 32, (1, 2, 2, 4), 5, 3, None),
                                           (6, 32, (1, 2, 4), 4, 2, 64), (6, 32, (1, 4, 2), 4, 2, None)):
        ckpt, w, _ = _synthetic_checkpoint(td, dim, mults, od, ad, time_dim=tdim)
        arch = infer_architecture(ckpt["model_state_dict"])
        assert arch["dim_mults"] == mults and arch["dim"] == dim and arch["transition_dim"] == td
        assert arch["time_dim"] == (tdim or dim) and arch["kernel_size"] == 5
        assert infer_architecture(w) == arch                       # bare TemporalUnet dict: same answer
        diff = load_checkpoint(ckpt, device="cpu")
        assert (diff.horizon, diff.observation_dim, diff.action_dim, diff.n_timesteps) == (32, od, ad, 20)
        assert diff.model.dim_mults == mults and not diff.training
        for k, v in w.items():
            assert torch.equal(diff.state_dict()["model." + k], torch.from_numpy(v)), k
        assert diff.loaded_from["state"] == "model_state_dict" and diff.loaded_from["epoch"] == 3
    # the real architectures' key schema (from the reference) resolves to the right widths
    for net, mults in (("halfcheetah", (1, 4, 8)), ("door", (1, 2, 4, 8)), ("pointmaze", (1, 2, 4))):
        shapes = {k: torch.empty(v, device="meta") for k, v in want[net]["model"].items()}
        assert infer_architecture(shapes)["dim_mults"] == mults
    # by path, EMA branch, overrides for config-less checkpoints
    ckpt, w, w_ema = _synthetic_checkpoint(6, 32, (1, 2, 4), 4, 2, ema_seed=9)
    path = tmp_path / "ckpt.pt"
    torch.save(ckpt, path)
    raw = load_checkpoint(str(path), device="cpu")
    ema = load_checkpoint(path, device="cpu", use_ema=True)
    key = "model.mid_block1.blocks.0.block.0.weight"
    assert torch.equal(raw.state_dict()[key], torch.from_numpy(w[key[6:]]))
    assert torch.equal(ema.state_dict()[key], torch.from_numpy(w_ema[key[6:]]))
    assert not torch.equal(raw.state_dict()[key], ema.state_dict()[key])
    old = {"model_state_dict": ckpt["model_state_dict"]}
    with pytest.raises(KeyError, match="horizon"):
        load_checkpoint(old, device="cpu")
    d = load_checkpoint(old, device="cpu", horizon=32, observation_dim=4, action_dim=2)
    assert d.beta_schedule == "cosine" and d.n_timesteps == 20
    with pytest.raises(KeyError, match="ema_state_dict"):
        load_checkpoint(old, device="cpu", use_ema=True, horizon=32, observation_dim=4, action_dim=2)
    with pytest.raises(ValueError, match="transition_dim"):
        load_checkpoint(old, device="cpu", horizon=32, observation_dim=5, action_dim=2)
    broken = dict(ckpt, model_state_dict={k: v for k, v in ckpt["model_state_dict"].items()
                                          if k != "model.ups.0.1.time_mlp.1.bias"})
    with pytest.raises(KeyError, match="ups.0.1.time_mlp.1.bias"):
        load_checkpoint(broken, device="cpu")
    extra = dict(ckpt, model_state_dict=dict(ckpt["model_state_dict"], **{"model.bogus.weight": torch.zeros(3)}))
    with pytest.raises(KeyError, match="bogus"):
        load_checkpoint(extra, device="cpu")
    with pytest.raises(KeyError, match="not a TemporalUnet"):
        infer_architecture({"betas": torch.zeros(4)})


# ------------------------------------------------------------------------------ projection
def test_projection_builder_matches_reference():
    from dynamics_aware_diffusion_amd.dynamics import ProjectionMatrixBuilder
    from oracle.projection import double_integrator, lifted_map
    g = golden("projection")
    for case, dt, Hh in cases.PROJ_MATRIX_CASES:
        A, B = double_integrator(dt)
        b = ProjectionMatrixBuilder(A, B, 4, 2)
        assert np.allclose(b._build_F_matrix(Hh), lifted_map(A, B, Hh), atol=0, rtol=0)
        P = b.get_projection_matrix(Hh)
        assert P.dtype == torch.float32 and P.shape == ((Hh + 1) * 4 + Hh * 2,) * 2
        assert max_abs(P.numpy(), g[case]) <= 1e-6
        assert b.verify_projection(P)
        assert np.linalg.matrix_rank(P.double().numpy(), tol=1e-6) == 4 + Hh * 2
    with pytest.raises(AssertionError):
        ProjectionMatrixBuilder(np.eye(3), np.zeros((4, 2)), 4, 2)


# ---------------------------------------------------------------------------- planner glue
class _FakeDiffusion(torch.nn.Module):
    horizon, observation_dim, action_dim, transition_dim, n_timesteps = 32, 4, 2, 6, 20

    def __init__(self):
        super().__init__()
        self.register_buffer("betas", torch.linspace(1e-4, 0.02, 20))


def test_action_buffer_and_observation_glue():
    from dynamics_aware_diffusion_amd import DynamicsAwarePolicy, GuidedPolicy, MPCPolicy
    norm = cases.NormalizerStub(4, 2)
    diff = _FakeDiffusion()
    traj = torch.from_numpy(np.arange(32 * 6, dtype=np.float32).reshape(1, 32, 6))
    for ah, expect in ((1, 2), (8, 9), (32, 32), (100, 32)):      # min(a + 1, H) entries
        pol = GuidedPolicy(diff, norm, action_horizon=ah)
        pol._fill_action_buffer(traj)
        assert len(pol.action_buffer) == expect
        want0 = norm.unnormalize_actions(traj[0, 0, 4:6].numpy().reshape(1, -1)).flatten()
        assert np.array_equal(pol.action_buffer[0], want0)        # starts at horizon step 0
        first = pol.get_action(np.zeros(4))                       # served from the buffer
        assert np.array_equal(first, want0) and len(pol.action_buffer) == expect - 1
    assert GuidedPolicy(diff, norm).action_horizon == 1
    assert MPCPolicy(diff, norm).action_horizon == 8
    assert DynamicsAwarePolicy(diff, normalizer=norm, horizon=32).action_horizon == 32
    pol = GuidedPolicy(diff, norm)
    obs = {"observation": np.arange(4.0), "desired_goal": np.ones(2), "achieved_goal": np.zeros(2)}
    assert pol._process_observation(obs).shape == (1, 4)           # state-only model
    pol6 = GuidedPolicy(diff, cases.NormalizerStub(6, 2))
    assert pol6._process_observation(obs).shape == (1, 6)          # goal-conditioned model
    assert pol._process_observation({"achieved_goal": np.ones(3)}).shape == (1, 3)
    assert pol._process_observation([1.0, 2.0, 3.0, 4.0]).shape == (1, 4)


def test_projection_alpha_schedules_match_reference():
    from dynamics_aware_diffusion_amd import DynamicsAwarePolicy
    from oracle.denoiser import schedule_buffers
    g = golden("projection")
    diff = _FakeDiffusion()
    diff.n_timesteps = 100
    diff.betas = schedule_buffers("cosine", 100)["betas"]
    for sched in cases.PROJ_SCHEDULES:
        pol = DynamicsAwarePolicy(diff, normalizer=cases.NormalizerStub(4, 2), horizon=32,
                                  projection_schedule=sched, projection_strength=cases.PROJ_STRENGTH)
        for t in cases.PROJ_T:
            assert abs(pol._get_projection_alpha(t) - float(g[f"alpha_{sched}_{t}"])) <= 1e-12
    # no projector or no normaliser: identity, as the reference (policies.py:422-423)
    pol = DynamicsAwarePolicy(diff, projection_matrix=None, normalizer=None, horizon=32)
    x = torch.zeros(2, 32, 6)
    assert pol.apply_projection(x, 3) is x


def test_sampler_refuses_cpu_tensors():
    from dynamics_aware_diffusion_amd import GaussianDiffusion, GuidedPolicy, TemporalUnet
    unet = TemporalUnet(6, dim=32, dim_mults=(1, 2))
    diff = GaussianDiffusion(unet, 32, 4, 2, n_timesteps=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        unet(torch.zeros(1, 32, 6), torch.zeros(1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diff.p_sample_loop((1, 32, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GuidedPolicy(diff, None).sample_loop(batch_size=1)
    with pytest.raises(NotImplementedError):             # one timestep per call
        TemporalUnet.shared_timestep(torch.tensor([1, 2]))


# -------------------------------------------------------------------------------- Philox
def test_philox_known_answers_and_moments():
    from oracle import philox
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]          # Random123 kat_vectors
    for ctr, key, want in kat:
        got = philox.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert got.tolist() == list(want)
    z = philox.normal(np.arange(400_000, dtype=np.uint64), draw=3, seed=12345)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and np.isfinite(z).all()
    assert not np.array_equal(z[:1000], philox.normal(np.arange(1000, dtype=np.uint64), 4, 12345))


# ------------------------------------------------------------------------------- sharding
def test_shard_ranges_cover_the_batch():
    from dynamics_aware_diffusion_amd.utils.sharding import shard_range
    for total in (0, 1, 7, 256, 1024, 1000):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, world, r) for r in range(world)]
            assert sum(c for _, c in spans) == total
            pos = 0
            for start, count in spans:
                assert start == pos
                pos += count
            assert max(c for _, c in spans) - min(c for _, c in spans) <= 1
    with pytest.raises(ValueError):
        shard_range(4, 2, 2)


_WORKER = r"""
import os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from dynamics_aware_diffusion_amd.utils import synth
from dynamics_aware_diffusion_amd.utils.sharding import gather_plans, sample_sharded, shard_range
rank, world, total = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(sys.argv[2])
dist.init_process_group("gloo", rank=rank, world_size=world)
full = torch.from_numpy(synth.normal_like(9, "shard.plans", (total, 32, 6)))

class StubPolicy:                       # rows are a pure function of the GLOBAL row index
    def sample_loop(self, batch_size, conditions=None, row_offset=0):
        out = full[row_offset:row_offset + batch_size].clone()
        if conditions is not None:
            out[:, 0] = conditions[0]
        return out

start, count = shard_range(total, world, rank)
got = gather_plans(full[start:start + count].clone(), total)
assert torch.equal(got, full), "gather order"
cond = torch.from_numpy(synth.normal_like(9, "shard.cond", (total, 6)))
got2 = sample_sharded(StubPolicy(), total, {0: cond})
want2 = full.clone(); want2[:, 0] = cond
assert torch.equal(got2, want2), "per-row conditions"
got3 = sample_sharded(StubPolicy(), total, {0: cond[:1]})
want3 = full.clone(); want3[:, 0] = cond[:1]
assert torch.equal(got3, want3), "broadcast condition"
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("world,total", [(2, 8), (2, 7), (8, 1024), (8, 21)],
                         ids=["w2_8", "w2_7ragged", "w8_1024_config5", "w8_21ragged"])
def test_sharded_gather_over_gloo(tmp_path, world, total):
    """CPU rehearsal of the multi-GPU path over gloo: shard -> sample -> gather, at world size 2 and at
    BASELINE config 5's shape (8 ranks x 128 = 1024 plans; equal shards: one all_gather_into_tensor) plus
    ragged splits."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + (total * 7 + world + os.getpid()) % 400),
               WORLD_SIZE=str(world), OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, str(total)],
                              env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{out}"
        assert f"rank {r} ok" in out


def test_bench_self_launch_starts_ranks_without_touching_the_gpu():
    """`python bench.py --gpus 2` with no launcher: the parent spawns the ranks (it never imports
    torch, let alone initialises a GPU) and exits with the launcher's code.  Here there is no GPU,
    so both ranks must fail loudly — which proves they were started and that failure propagates."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
                          "--warmup", "0", "--no-configs"], env=env, capture_output=True, text=True,
                         timeout=600)
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by the -m gpu rehearsal test")
    assert run.returncode != 0
    assert "needs a ROCm device" in run.stderr
    assert "--gpus 2 needs torch.distributed.run" not in run.stderr


# --------------------------------------------------------------- dynamics package
def _synthetic_transitions(n_obs=6, n=4, m=2, N=400, noise=0.0, seed=3):
    from dynamics_aware_diffusion_amd.dynamics import double_integrator
    A, B = double_integrator(0.1)
    rng = np.random.default_rng(seed)
    S = rng.normal(size=(N, n_obs))
    U = rng.normal(size=(N, m))
    S1 = rng.normal(size=(N, n_obs))                     # goal columns: unrelated to the dynamics
    S1[:, :n] = S[:, :n] @ A.T + U @ B.T + noise * rng.normal(size=(N, n))
    return A, B, S, U, S1


def test_least_squares_fit_recovers_the_linear_system():
    """data_driven.py:75-134: lstsq on [X U]; state_dim keeps the physical columns."""
    from dynamics_aware_diffusion_amd.dynamics import fit_linear_dynamics, identify_dynamics_from_arrays
    A, B, S, U, S1 = _synthetic_transitions()
    A2, B2, q = fit_linear_dynamics(S, U, S1, state_dim=4, return_quality=True)
    assert np.abs(A2 - A).max() <= 1e-12 and np.abs(B2 - B).max() <= 1e-12
    assert q["r_squared"] > 1 - 1e-12 and q["mean_prediction_error"] < 1e-12
    # the same numbers as numpy's lstsq on the stacked regressors (the reference's formulation)
    theta = np.linalg.lstsq(np.hstack([S[:, :4], U]), S1[:, :4], rcond=None)[0]
    assert np.array_equal(A2, theta[:4].T) and np.array_equal(B2, theta[4:].T)
    A3, B3, n, m = identify_dynamics_from_arrays(S, U, S1, state_dim=4)
    assert (n, m) == (4, 2) and np.array_equal(A3, A2)
    # full observation when no state_dim is given (6 x 6 system)
    A6, B6 = fit_linear_dynamics(S, U, S1)
    assert A6.shape == (6, 6) and B6.shape == (6, 2)
    with pytest.raises(ValueError):
        fit_linear_dynamics(S, U[:-1], S1)
    with pytest.raises(ValueError):
        fit_linear_dynamics(S[:3], U[:3], S1[:3])


def test_registry_and_episode_helpers():
    from dynamics_aware_diffusion_amd import dynamics as dyn
    assert dyn.state_dim_for_env("PointMaze_UMaze-v3") == 4
    assert dyn.state_dim_for_env("HalfCheetah-v5") == 17
    assert dyn.state_dim_for_env("AdroitHandDoor-v1") is None          # full observation (n = 39)
    A, B, n, m = dyn.get_dynamics_for_env("PointMaze_UMaze-v3")        # no data: analytical model
    A0, B0 = dyn.double_integrator(0.1)
    assert (n, m) == (4, 2) and np.array_equal(A, A0) and np.array_equal(B, B0)
    At, Bt, S, U, S1 = _synthetic_transitions()
    A2, B2, n2, m2 = dyn.get_dynamics_for_env("pointmaze", transitions=(S, U, S1))
    assert (n2, m2) == (4, 2) and np.abs(A2 - At).max() <= 1e-12
    with pytest.raises(ValueError):
        dyn.get_dynamics_for_env("HalfCheetah-v5")                     # needs data
    with pytest.raises(ImportError):
        dyn.identify_dynamics_from_data("D4RL/pointmaze/umaze-v2")
    obs = [np.arange(12.0).reshape(4, 3), np.arange(9.0).reshape(3, 3)]
    act = [np.ones((3, 2)), np.ones((2, 2))]
    s, a, s1 = dyn.transitions_from_episodes(obs, act, state_dim=2)
    assert s.shape == (5, 2) and a.shape == (5, 2) and np.array_equal(s1[0], obs[0][1, :2])
    with pytest.raises(ValueError):
        dyn.transitions_from_episodes([np.zeros((3, 3))], [np.zeros((3, 2))])


def test_qr_projector_equals_the_pinv_projector():
    """The device path's algorithm (P = Q Q^T) against the reference's F pinv(F), on the CPU."""
    from dynamics_aware_diffusion_amd.dynamics import ProjectionMatrixBuilder, double_integrator
    A, B = double_integrator(0.1)
    b = ProjectionMatrixBuilder(A, B, 4, 2)
    for H in (8, 32):
        assert float((b.projection_matrix_on_device(H, "cpu") - b.get_projection_matrix(H)).abs().max()) <= 1e-6
    rng = np.random.default_rng(5)
    A = 0.9 * np.linalg.qr(rng.normal(size=(7, 7)))[0]
    B = rng.normal(size=(7, 3))
    b = ProjectionMatrixBuilder(A, B, 7, 3)
    P = b.projection_matrix_on_device(16, "cpu")
    assert float((P - b.get_projection_matrix(16)).abs().max()) <= 1e-6 and b.verify_projection(P)


def test_deepcopy_and_pickle_leave_the_engine_behind():
    """The reference's trainer keeps EMA weights in ``copy.deepcopy(model)`` (utils/training.py:77): a copy of the
    model gets parameters and options but no ``dad_model`` handle (ctypes pointers cannot be copied; the copy builds
    its own engine on its first call), and the cached parameter walk follows the copy's own Parameters."""
    import copy
    import ctypes
    import pickle
    from dynamics_aware_diffusion_amd import GaussianDiffusion, TemporalUnet
    unet = TemporalUnet(6, dim=32, dim_mults=(1, 2))
    diff = GaussianDiffusion(unet, 8, 4, 2, n_timesteps=10)
    unet._engine = ctypes.c_void_p(5)          # stands for a built engine: not copyable
    unet.precision = "f16x3"
    assert len(unet._params()) == len(list(unet.parameters()))
    twin = copy.deepcopy(diff)
    assert twin.model._engine is None and twin.model._engine_sig is None and twin.model.precision == "f16x3"
    mine, theirs = dict(unet.named_parameters()), twin.model._params()
    assert set(mine) == set(theirs)
    assert all(torch.equal(mine[k], theirs[k]) and mine[k] is not theirs[k] for k in mine)
    assert all(theirs[k] is p for k, p in twin.model.named_parameters())
    with torch.no_grad():                       # an EMA update of the copy does not touch the original
        for k in theirs:
            theirs[k].mul_(0.5)
    assert all(torch.equal(mine[k] * 0.5, theirs[k]) for k in mine)
    unet._engine = None
    back = pickle.loads(pickle.dumps(unet))
    assert torch.equal(back.state_dict()["final_conv.1.weight"], unet.state_dict()["final_conv.1.weight"])
