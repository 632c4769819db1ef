"""ctypes binding of ``libdad_hip.so`` (C ABI: ``include/dad.h``) and the thin engine object
the API mirror classes drive.

There is deliberately NO fallback: if the library is missing or a tensor is not on a ROCm
device the calls raise.  torch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import os
import weakref
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DAD_LIB selects an alternative build of the same ABI (timing-only ablation builds).
LIB_PATH = os.environ.get("DAD_LIB") or os.path.join(_HERE, "libdad_hip.so")

DAD_MAX_LEVELS = 8


class DadCfg(C.Structure):
    _fields_ = [
        ("transition_dim", C.c_int32), ("dim", C.c_int32), ("time_dim", C.c_int32),
        ("n_levels", C.c_int32), ("channels", C.c_int32 * DAD_MAX_LEVELS),
        ("kernel_size", C.c_int32), ("horizon", C.c_int32), ("n_timesteps", C.c_int32),
        ("predict_epsilon", C.c_int32), ("clip_denoised", C.c_int32),
    ]


class DadStepArgs(C.Structure):
    _fields_ = [
        ("noise", C.c_void_p), ("seed", C.c_uint64), ("row_offset", C.c_uint64),
        ("draw", C.c_uint64), ("cond0", C.c_void_p), ("cond_per_row", C.c_int32),
        ("guide_grad", C.c_void_p), ("guide_weight", C.c_float),
        ("mean_out", C.c_void_p), ("eps_out", C.c_void_p),
    ]


class DadSamplerCoef(C.Structure):
    _fields_ = [("t", C.c_int32)] + [(k, C.c_float) for k in (
        "c_recip", "c_recipm1", "guide_x0", "coef_x0", "coef_xt", "guide_mean", "sigma")]


SAMPLER_COEF_FIELDS = tuple(name for name, _ in DadSamplerCoef._fields_[1:])
# numpy view of an array of dad_sampler_coef (32 bytes, no padding)
SAMPLER_COEF_DTYPE = np.dtype([("t", "<i4")] + [(k, "<f4") for k in SAMPLER_COEF_FIELDS])


def pack_sampler_steps(table: Mapping[str, "np.ndarray"], order: Optional[Sequence[int]] = None) -> "np.ndarray":
    """Rows ``order`` (default: all, as given) of a coefficient table such as ``models.diffusion.ddim_table``
    returns — ``tau`` and one float64 array per field of ``dad_sampler_coef`` — as an array of that struct.  This is
    the one rounding to fp32."""
    tau = np.asarray(table["tau"], dtype=np.int64)
    idx = np.arange(tau.shape[0]) if order is None else np.asarray(order, dtype=np.int64)
    out = np.zeros(idx.shape[0], dtype=SAMPLER_COEF_DTYPE)
    out["t"] = tau[idx]
    for k in SAMPLER_COEF_FIELDS:
        out[k] = np.asarray(table[k], dtype=np.float64)[idx]
    return out


def _steps_array(steps, what: str) -> "np.ndarray":
    arr = np.ascontiguousarray(steps)
    if arr.dtype != SAMPLER_COEF_DTYPE or arr.ndim != 1:
        raise TypeError(f"{what} must be a 1-d array of SAMPLER_COEF_DTYPE (pack_sampler_steps)")
    return arr


class DadProjectArgs(C.Structure):
    _fields_ = [
        ("P", C.c_void_p), ("obs_mean", C.c_void_p), ("obs_std", C.c_void_p),
        ("act_mean", C.c_void_p), ("act_std", C.c_void_p),
        ("state_dim", C.c_int32), ("observation_dim", C.c_int32), ("action_dim", C.c_int32),
        ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
    ]


DAD_GUIDE_MAX_LAYERS = 4


class DadGuideArgs(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int32), ("in_dim", C.c_int32),
        ("widths", C.c_int32 * DAD_GUIDE_MAX_LAYERS), ("padded", C.c_int32 * DAD_GUIDE_MAX_LAYERS),
        ("activation", C.c_int32),
        ("w_fwd", C.c_void_p * DAD_GUIDE_MAX_LAYERS), ("w_bwd", C.c_void_p * DAD_GUIDE_MAX_LAYERS),
        ("bias", C.c_void_p * DAD_GUIDE_MAX_LAYERS),
        ("grad", C.c_void_p), ("grad_bytes", C.c_size_t),
    ]


class DadOptimTensor(C.Structure):
    _fields_ = [
        ("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("ema", C.c_void_p), ("numel", C.c_int64), ("group", C.c_int32),
    ]


class DadOptimGroup(C.Structure):
    _fields_ = [
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("weight_decay", C.c_float), ("step_size", C.c_float), ("bc2_sqrt", C.c_float),
        ("decoupled", C.c_int32), ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float),
    ]


class DadOptimArgs(C.Structure):
    _fields_ = [
        ("groups", C.POINTER(DadOptimGroup)), ("n_groups", C.c_int32), ("max_grad_norm", C.c_float),
        ("ema_decay", C.c_float), ("grad_norm_out", C.c_void_p),
    ]


OPTIM_MAX_GROUPS = 8


# name -> (restype, argtypes); also the list of symbols include/dad.h declares.
ABI = {
    "dad_last_error": (C.c_char_p, []),
    "dad_version": (C.c_char_p, []),
    "dad_model_create": (C.c_int, [C.POINTER(DadCfg), C.POINTER(C.c_void_p)]),
    "dad_model_destroy": (None, [C.c_void_p]),
    "dad_model_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p,
                                        C.POINTER(C.c_int64), C.c_int32]),
    "dad_model_load_schedule": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "dad_model_load_time_embedding": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "dad_model_set_precision": (C.c_int, [C.c_void_p, C.c_int32]),
    "dad_model_set_group_channels": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "dad_model_set_horizon": (C.c_int, [C.c_void_p, C.c_int32]),
    "dad_model_finalize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "dad_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t)]),
    "dad_unet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_unet_forward_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_projection_violation": (C.c_int, [C.POINTER(DadProjectArgs), C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_int32, C.c_void_p]),
    "dad_violation_grad_workspace_bytes": (C.c_int, [C.POINTER(DadProjectArgs), C.c_int32, C.c_int32, C.c_int32,
                                                     C.POINTER(C.c_size_t)]),
    "dad_projection_violation_fwd": (C.c_int, [C.POINTER(DadProjectArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dad_projection_violation_bwd": (C.c_int, [C.POINTER(DadProjectArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                               C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "dad_debug_violation_grad_plan": (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32)]),
    "dad_denoise_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.POINTER(DadStepArgs), C.c_int32, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "dad_sample_loop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32,
                                  C.POINTER(DadProjectArgs), C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "dad_sampler_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.POINTER(DadStepArgs), C.c_int32, C.c_void_p, C.c_size_t,
                                   C.c_void_p]),
    "dad_sampler_loop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32,
                                   C.POINTER(DadProjectArgs), C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "dad_guide_grad": (C.c_int, [C.POINTER(DadGuideArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                 C.c_int32, C.c_void_p]),
    "dad_guided_loop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_uint64, C.c_uint64, C.c_void_p, C.c_int32,
                                  C.POINTER(DadGuideArgs), C.c_float,
                                  C.POINTER(DadProjectArgs), C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_size_t, C.c_void_p]),
    "dad_debug_guide_plan": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.POINTER(C.c_int32)]),
    "dad_project": (C.c_int, [C.POINTER(DadProjectArgs), C.c_float, C.c_void_p, C.c_int32,
                              C.c_int32, C.c_void_p]),
    "dad_fill_normal": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                  C.c_uint64, C.c_void_p]),
    "dad_debug_set_tile": (C.c_int, [C.c_void_p, C.c_int32]),
    "dad_debug_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "dad_debug_read_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.POINTER(C.c_int32)]),
    "dad_debug_mish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "dad_debug_kernel_table_consistent": (C.c_int, []),
    "dad_debug_small_batch_plan": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
    "dad_debug_backward_plan": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                          C.POINTER(C.c_int32)]),
    "dad_debug_backward_steps": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                           C.POINTER(C.c_int32)]),
    "dad_model_set_training": (C.c_int, [C.c_void_p, C.c_int32]),
    "dad_model_refresh_weights": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p),
                                            C.c_void_p]),
    "dad_train_grad_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "dad_train_grad_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64)]),
    "dad_train_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_size_t)]),
    "dad_unet_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_unet_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(C.c_void_p), C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_model_load_train_schedule": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "dad_train_time_grad_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "dad_train_time_grad_info": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int64)]),
    "dad_train_objective_workspace_bytes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t),
                                                      C.POINTER(C.c_size_t)]),
    "dad_train_objective_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_train_objective_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.c_int32,
                                               C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_train_dynamics_objective_workspace_bytes": (C.c_int, [C.c_void_p, C.POINTER(DadProjectArgs), C.c_int32, C.c_int32,
                                                               C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "dad_train_dynamics_objective_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                       C.POINTER(DadProjectArgs), C.c_int32, C.c_int32, C.c_float, C.c_float,
                                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_train_dynamics_objective_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                        C.POINTER(DadProjectArgs), C.c_int32, C.c_int32, C.c_float, C.c_float,
                                                        C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32,
                                                        C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_void_p, C.c_size_t,
                                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "dad_debug_dynamics_objective_plan": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.POINTER(C.c_int32), C.c_int32,
                                                                                      C.POINTER(C.c_int32)]),
    "dad_debug_objective_offsets": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "dad_debug_objective_plan": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                           C.POINTER(C.c_int32)]),
    "dad_debug_forward_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                         C.POINTER(C.c_int32)]),
    "dad_debug_halo8_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                       C.POINTER(C.c_int32)]),
    "dad_debug_project_plan": (C.c_int, [C.c_int32] * 5 + [C.c_size_t, C.c_int32, C.POINTER(C.c_int32)]),
    "dad_debug_seam_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "dad_debug_seam_reason": (C.c_char_p, [C.c_int32]),
    "dad_debug_kernel_list": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    "dad_debug_report_layout": (C.c_char_p, [C.c_int32, C.c_int32]),
    "dad_optim_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "dad_optim_destroy": (None, [C.c_void_p]),
    "dad_optim_step": (C.c_int, [C.c_void_p, C.POINTER(DadOptimTensor), C.c_int32, C.POINTER(DadOptimArgs), C.c_void_p]),
    "dad_debug_optim_plan": (C.c_int, [C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                       C.POINTER(C.c_int32)]),
    "dad_profile_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "dad_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_double)]),
}

_lib = None


def load_library() -> C.CDLL:
    """Load libdad_hip.so and type every entry point.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with dynamics_aware_diffusion_amd/csrc/build.sh "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():
        if os.environ.get("DAD_LIB") and not hasattr(lib, name):
            continue                       # an older timing-only build (A/B of two libraries on one box)
        fn = getattr(lib, name)            # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


class DadError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libdad_hip error {code}: {message}")
        self.code = code


def _check(lib, rc: int) -> None:
    if rc != 0:
        # DadError is a RuntimeError: DAD_E_RANGE (timestep outside the schedule) therefore surfaces
        # as the same exception type the reference's gather raises (diffusion.py:28)
        raise DadError(rc, lib.dad_last_error().decode("utf-8", "replace"))


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a ROCm device (got {t.device}); the HIP engine "
                           "has no CPU path")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous float32 (got {t.dtype}, "
                           f"contiguous={t.is_contiguous()})")


PRECISIONS = {"fp32": 0, "f16x3": 1}      # DAD_PREC_* of include/dad.h
LOSS_TYPES = {"l1": 1, "l2": 2}           # DAD_LOSS_* of include/dad.h
TABLES = {"sinusoid": 0, "time_mlp": 1, "blocks": 2}      # DAD_TABLE_* of include/dad.h
FP_FLAGS = ("x3", "bdir", "ragged", "res", "padded", "windowed")      # bits 0..5 of a record's flag word

# ---------------------------------------------------------------------- plan reports
# The debug queries return flat int32 vectors whose layouts include/dad.h states once (its *_LIST lists).  Nothing of a
# layout is written down here: the library hands the lists over as text, and reports are decoded by name.
@functools.lru_cache(None)
def report_layouts() -> dict:
    """Every section of every plan report as the library states it (dad_debug_report_layout: static text, no model, no
    device), asked on first use: {the constant that holds the section's length: ((constant, name, span), ...)}.
    Sections are headers, records and the names of the values a field takes."""
    lib, found = load_library(), {}
    for report, section in ((r, s) for r in range(64) for s in range(64)):      # (NULL outside the table, which is smaller)
        text = lib.dad_debug_report_layout(report, section)
        if text is not None:
            length, *f = text.decode().split()
            found[length] = tuple(zip(f[0::3], f[1::3], map(int, f[2::3])))
    return found


@functools.lru_cache(None)
def _fields(section: str):
    """(((name, offset, span), ...) of the fields a section reports — the reserved ones, "_", left out —, its length)."""
    at, fields = 0, []
    for _, name, span in report_layouts()[section]:
        if name != "_":
            fields.append((name, at, span))
        at += span
    return tuple(fields), at


def _names(section: str) -> tuple:
    """A section's names in order: a record's fields, or the names of a field's values (value = position)."""
    return tuple(name for name, _, _ in _fields(section)[0])


def _decode(section: str, ints, at: int = 0) -> dict:
    """The ints from `at` on by the names of `section`: an int per field, a list for a field that spans several."""
    return {name: ints[at + o] if span == 1 else list(ints[at + o:at + o + span]) for name, o, span in _fields(section)[0]}


def decode_report(ints, header: str, record):
    """(header dict, [one dict per record]) of a report's ints.  `header` and `record` name the sections by their length
    constants; with several kinds of record, `record` is a function (header dict, where a record starts) -> section."""
    head = _decode(header, ints)
    k = head.pop("record_ints")
    recs = []
    for at in range(_fields(header)[1], len(ints), k):
        section = record(head, at) if callable(record) else record
        assert _fields(section)[1] == k and at + k <= len(ints)
        recs.append(_decode(section, ints, at))
    return head, recs


def _fetch(fn, *args) -> list:
    """The two calls of every sized report: ask how many ints there are, then fetch them."""
    lib, need = load_library(), C.c_int32()
    _check(lib, fn(*args, None, 0, C.byref(need)))
    out = (C.c_int32 * need.value)()
    _check(lib, fn(*args, out, need.value, C.byref(need)))
    return list(out)


def __getattr__(name: str):
    """Value names other modules import, served from the library's lists on first use."""
    sections = {"TIME_GEMM_MODES": "DAD_OP_TG_MODES", "KERNEL_FAMILIES": "DAD_FAMILIES"}
    if name in sections:
        return _names(sections[name])
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def kernel_list(family: str):
    """The keys of one family of instantiated kernels in the library's own registry, the table every launch looks its
    kernel up in (dad_debug_kernel_list), as a set of tuples; host logic only."""
    out = _fetch(load_library().dad_debug_kernel_list, _names("DAD_FAMILIES").index(family))
    head, start = _decode("DAD_KL_HEADER", out), _fields("DAD_KL_HEADER")[1]
    ints = head["key_ints"]
    assert len(out) - start == head["kernels"] * ints
    return {tuple(out[at:at + ints]) for at in range(start, len(out), ints)}


def registered_kernels():
    """Every kernel key of the conv-GEMM and the small-batch families in the library's registry, in the form
    HipEngine.forward_plan reports them: ("gemm", cfg, taps, stride, flags), ("cc", taps, stride, ride, big, rows, windowed),
    ("ccw", taps, stride, ride, ride_in, rows).  Returns (gemm keys, cc keys, ccw keys) as sets; host logic only."""
    return tuple({(family,) + k for k in kernel_list(family)} for family in ("gemm", "cc", "ccw"))


def fullchip_kernels():
    """Every instantiation of the two full-chip families in the library's registry: ({("halo8", cfg, ride)},
    {("seam", dim, tile0)}); host logic only."""
    return tuple({(family,) + k for k in kernel_list(family)} for family in ("halo8", "seam"))


BS_WRITES = ("set", "add", "stage")       # BwdWrite of csrc/host_plan.hpp


def wgrad_kernels():
    """Every (taps, tile, windowed) of the conv_wgrad family in the library's registry; host logic only."""
    return kernel_list("wgrad")


def projection_plan(state_dim: int, observation_dim: int, action_dim: int, batch: int, horizon: int, *,
                    scratch_bytes: int = 0, violation: bool = False) -> dict:
    """Which kernel one dad_project (or, ``violation``, dad_projection_violation) call launches at this shape with a
    scratch copy of ``scratch_bytes`` (0: none), and on which grid (dad_debug_project_plan: the plan the entry points
    launch from; host logic only).  Returns ``form`` ("row1", "row4" or "gemm"), ``rows_per_block``, ``grid`` (x, y),
    ``lds_bytes`` and ``refused`` (the call fails: the row does not fit LDS and the GEMM form is not to be had)."""
    lib = load_library()
    out = (C.c_int32 * _fields("DAD_PP_INTS")[1])()
    _check(lib, lib.dad_debug_project_plan(int(state_dim), int(observation_dim), int(action_dim), int(batch), int(horizon),
                                           int(scratch_bytes), int(bool(violation)), out))
    q = _decode("DAD_PP_INTS", out)
    q["form"], q["refused"] = _names("DAD_PP_FORMS")[q["form"]], bool(q["refused"])
    q["grid"] = (q.pop("gx"), q.pop("gy"))
    return q


VIOLATION_FORMS = {None: -1, "row": 0, "gemm": 1}      # the `form` argument of dad_projection_violation_fwd / _bwd


def _violation_form(form) -> int:
    if form not in VIOLATION_FORMS:
        raise ValueError(f"form must be None (planned), \"row\" or \"gemm\", got {form!r}")
    return VIOLATION_FORMS[form]


def violation_grad_plan(state_dim: int, observation_dim: int, action_dim: int, batch: int, horizon: int,
                        form: Optional[str] = None) -> dict:
    """What one dad_projection_violation_fwd / _bwd pair launches at this shape under ``form`` (None: the planner's
    choice, "row", "gemm"), decoded by name (dad_debug_violation_grad_plan: the plan the entry points launch from; host
    logic only).  ``form`` comes back as "row" or "gemm"; ``fwd`` and ``bwd`` each hold ``rows_per_block``, ``grid``
    (x, y), ``lds_bytes`` and the blocks of the pass's small second launch (``sum_gx`` / ``scatter_gx``, 0 in the row
    form); ``workspace_bytes``; ``refused`` (a forced row form whose row does not fit LDS: the calls fail)."""
    lib = load_library()
    out = (C.c_int32 * _fields("DAD_VG_INTS")[1])()
    _check(lib, lib.dad_debug_violation_grad_plan(int(state_dim), int(observation_dim), int(action_dim), int(batch),
                                                  int(horizon), _violation_form(form), out))
    q = _decode("DAD_VG_INTS", out)
    plan = {"form": _names("DAD_VG_FORMS")[q.pop("form")], "refused": bool(q.pop("refused")),
            "workspace_bytes": q.pop("workspace_bytes")}
    for side in ("fwd", "bwd"):
        d = {k[len(side) + 1:]: q.pop(k) for k in list(q) if k.startswith(side + "_")}
        d["grid"] = (d.pop("gx"), d.pop("gy"))
        plan[side] = d
    assert not q, q
    return plan


def guide_plan(in_dim: int, widths: Sequence[int], activation, batch: int, horizon: int,
               transition_dim: Optional[int] = None) -> dict:
    """What one guide launch (dad_guide_grad, and every guide launch of dad_guided_loop) is for the value net
    in_dim -> widths[0] -> ... -> widths[-1] with ``activation`` ("tanh", "relu", "mish", or the library's code) on
    trajectories (batch, horizon, transition_dim; default in_dim), decoded by name (dad_debug_guide_plan: the plan the
    entry points launch from and the one statement of the limits; host logic only).  ``padded``: the zero-padded in_dim
    and hidden widths, ``rows_per_block``, ``threads``, ``grid``, ``lds_bytes``, and ``refused``: None, or the name of
    the first limit the net misses ("layers", "width", "activation", "in_dim", "last_width", "lds")."""
    lib = load_library()
    acts = _names("DAD_GD_ACTS")
    code = acts.index(activation) if activation in acts else activation if isinstance(activation, int) else -1
    n = len(widths)
    w = (C.c_int32 * max(n, 1))(*[int(v) for v in widths])
    out = (C.c_int32 * _fields("DAD_GD_INTS")[1])()
    _check(lib, lib.dad_debug_guide_plan(int(in_dim), w, n, int(code), int(batch), int(horizon),
                                         int(in_dim if transition_dim is None else transition_dim), out))
    q = _decode("DAD_GD_INTS", out)
    hidden = max(min(n, DAD_GUIDE_MAX_LAYERS) - 1, 0)
    q["padded"] = [q.pop("padded_in")] + [q.pop(f"padded_{i}") for i in (1, 2, 3)][:hidden]
    for k in ("padded_1", "padded_2", "padded_3"):
        q.pop(k, None)
    q["grid"] = q.pop("gx")
    q["refused"] = None if q["refused"] == 0 else _names("DAD_GD_REFUSALS")[q["refused"]]
    return q


def optim_plan(numel: Sequence[int]) -> dict:
    """The work split of one optimiser step over tensors of these sizes (dad_debug_optim_plan; host logic only):
    chunk size, chunks, grid, partials and one record per chunk, with ``first`` as the whole element index."""
    sizes = (C.c_int64 * max(len(numel), 1))(*[int(v) for v in numel])
    head, recs = decode_report(_fetch(load_library().dad_debug_optim_plan, sizes, len(numel)), "DAD_OS_HEADER", "DAD_OS_REC_INTS")
    assert head["chunks"] == len(recs)
    for r in recs:
        r["first"] += r.pop("first_hi") << 31
    head["records"] = recs
    return head


def sinusoid_table(n_timesteps: int, dim: int) -> torch.Tensor:
    """SinusoidalPosEmb for t = 0 .. n_timesteps-1 with the reference's own torch expression
    (/root/reference/m_diffuser/models/temporal_unet.py:27-31), on the host: (n_timesteps, dim)
    fp32, bit-identical to what the reference's module computes on this machine."""
    half = dim // 2
    scale = math.log(10000) / (half - 1)
    freqs = torch.exp(torch.arange(half) * -scale)
    arg = torch.arange(n_timesteps)[:, None] * freqs[None, :]
    return torch.cat((arg.sin(), arg.cos()), dim=-1).contiguous()

SCHEDULE_KEYS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                 "posterior_mean_coef1", "posterior_mean_coef2",
                 "posterior_log_variance_clipped")


class HipEngine:
    """One ``dad_model`` on one device: packed weights, time tables, workspaces."""

    def __init__(self, *, transition_dim: int, dim: int, channels: Sequence[int], horizon: int,
                 n_timesteps: int, time_dim: Optional[int] = None, kernel_size: int = 5,
                 predict_epsilon: bool = True, clip_denoised: bool = True,
                 device: torch.device | str = "cuda", precision: str = "fp32", training: bool = False):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self.lib = load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HipEngine needs a ROCm device; there is no CPU path")
        # widths the tiles cannot hold (not a multiple of 32 with a power-of-two C / 8) run zero-padded:
        # utils/padding.py builds the padded tensors, the library is told the real widths
        from .utils import padding
        self.real_dim, self.real_channels = int(dim), [int(c) for c in channels]
        padded = [padding.padded_width(c) for c in self.real_channels]
        self.padded = padded != self.real_channels
        if self.padded:
            if self.real_channels[0] != self.real_dim:
                raise NotImplementedError("zero-padded widths need dim_mults[0] == 1")
            if transition_dim == self.real_dim:
                raise NotImplementedError(
                    f"transition_dim == dim == {dim} makes the first block's residual the trajectory itself; "
                    "with zero-padded GroupNorm groups that identity has no kernel")
        # horizons every level can halve but that are not a power of two (24, 48, 96, 100 ...) run zero-padded to
        # the next power of two (dad_model_set_horizon); the trajectory tensors keep their real shape
        horizon = int(horizon)
        levels = len(self.real_channels)
        # (... and the deepest level keeps at least four padded positions, the tiles' lower bound: horizon 16 on four
        # levels — 16 / 8 / 4 / 2 positions — runs in 32 / 16 / 8 / 4)
        self.padded_horizon = max(1 << max(horizon - 1, 0).bit_length(), 4 << (levels - 1))
        self.rows_padded = self.padded_horizon != horizon
        if self.rows_padded:
            if horizon % (1 << (levels - 1)) != 0:
                raise ValueError(f"horizon {horizon} cannot be halved {levels - 1} times (the reference's U-Net needs "
                                 f"H % 2^(levels-1) == 0, temporal_unet.py:35-54)")
            if transition_dim == self.real_dim:
                raise NotImplementedError("transition_dim == dim with a zero-padded horizon has no kernel")
        self.padded = self.padded or self.rows_padded
        cfg = DadCfg()
        cfg.transition_dim = transition_dim
        cfg.dim = padded[0] if padded != self.real_channels else dim
        cfg.time_dim = time_dim or dim
        cfg.n_levels = len(channels)
        for i, ch in enumerate(padded):
            cfg.channels[i] = int(ch)
        cfg.kernel_size = kernel_size
        cfg.horizon = self.padded_horizon
        cfg.n_timesteps = n_timesteps
        cfg.predict_epsilon = int(predict_epsilon)
        cfg.clip_denoised = int(clip_denoised)
        self.cfg = cfg
        self.horizon = horizon
        self.transition_dim = transition_dim
        self.n_timesteps = n_timesteps
        handle = C.c_void_p()
        _check(self.lib, self.lib.dad_model_create(C.byref(cfg), C.byref(handle)))
        self._h = handle
        _check(self.lib, self.lib.dad_model_set_precision(self._h, PRECISIONS[precision]))
        self.widths_padded = padded != self.real_channels
        if self.widths_padded:
            real = (C.c_int32 * len(self.real_channels))(*self.real_channels)
            _check(self.lib, self.lib.dad_model_set_group_channels(self._h, real, len(self.real_channels)))
        if self.rows_padded:
            _check(self.lib, self.lib.dad_model_set_horizon(self._h, horizon))
        self.training = bool(training)
        if self.training:
            _check(self.lib, self.lib.dad_model_set_training(self._h, 1))
        self._ws: Dict[int, torch.Tensor] = {}
        self._pinned: Dict[tuple, torch.Tensor] = {}
        self.ready = False

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self.lib.dad_model_destroy(h)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------ weights
    def load(self, unet_state: Mapping[str, torch.Tensor],
             schedule: Mapping[str, torch.Tensor]) -> None:
        """Upload every denoiser tensor (reference state_dict keys without ``model.``) and
        the five schedule buffers, then build tables and the launch plan."""
        if self.widths_padded:
            from .utils import padding
            mults = [c // self.real_dim for c in self.real_channels]
            self._pad_plan, _, _ = padding.padding_plan(unet_state.keys(), self.transition_dim, self.real_dim, mults)
            unet_state, _, _ = padding.pad_unet_state(unet_state, self.transition_dim, self.real_dim, mults)
        keep = []
        for key, t in unet_state.items():
            h = t.detach().to("cpu", torch.float32).contiguous()
            keep.append(h)
            shape = (C.c_int64 * h.dim())(*h.shape)
            _check(self.lib, self.lib.dad_model_load_weight(
                self._h, key.encode(), h.data_ptr(), shape, h.dim()))
        bufs = []
        for k in SCHEDULE_KEYS:
            b = schedule[k].detach().to("cpu", torch.float32).contiguous()
            if b.numel() != self.n_timesteps:
                raise ValueError(f"schedule buffer {k} has {b.numel()} entries, expected "
                                 f"{self.n_timesteps}")
            bufs.append(b)
        _check(self.lib, self.lib.dad_model_load_schedule(self._h, *[b.data_ptr() for b in bufs]))
        emb = sinusoid_table(self.n_timesteps, self.real_dim)
        if self.widths_padded:             # the real columns in front, as time_mlp.1.weight is padded
            wide = torch.zeros(self.n_timesteps, int(self.cfg.dim))
            wide[:, :self.real_dim] = emb
            emb = wide.contiguous()
        _check(self.lib, self.lib.dad_model_load_time_embedding(
            self._h, emb.data_ptr(), self.n_timesteps, int(self.cfg.dim)))
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_model_finalize(self._h, self._stream()))
        self.ready = True

    # ------------------------------------------------------------------ helpers
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def workspace(self, batch: int) -> torch.Tensor:
        """Device scratch for `batch` rows (activations + split-K slabs); grown on demand."""
        n = C.c_size_t()
        _check(self.lib, self.lib.dad_workspace_bytes(self._h, batch, C.byref(n)))
        ws = self._ws.get(batch)
        if ws is None or ws.numel() * 4 < n.value:
            ws = torch.empty(max(n.value, 4) // 4 + 4, dtype=torch.float32, device=self.device)
            self._ws[batch] = ws
        return ws

    def persistent(self, tag: str, shape) -> torch.Tensor:
        """A device tensor with a stable address per (tag, shape): hipGraph replays freeze the
        pointers they were captured with."""
        key = (tag, tuple(shape))
        t = self._pinned.get(key)
        if t is None:
            t = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
            self._pinned[key] = t
        return t

    def _traj(self, x: torch.Tensor, name: str = "x") -> int:
        _require_device(x, name)
        if x.dim() != 3 or x.shape[1] != self.horizon or x.shape[2] != self.transition_dim:
            raise RuntimeError(f"{name} must be (B, {self.horizon}, {self.transition_dim}), "
                               f"got {tuple(x.shape)}")
        return int(x.shape[0])

    # ------------------------------------------------------------------ compute
    def unet_forward(self, x: torch.Tensor, t: int) -> torch.Tensor:
        B = self._traj(x)
        out = torch.empty_like(x)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_unet_forward(
                self._h, x.data_ptr(), int(t), out.data_ptr(), B, ws.data_ptr(),
                ws.numel() * 4, self._stream()))
        return out

    def unet_forward_rows(self, x: torch.Tensor, t_rows: torch.Tensor) -> torch.Tensor:
        """eps_theta(x, t) with one timestep per row (the training objective's call); ``t_rows``
        is range-checked by the caller (``TemporalUnet.forward``)."""
        B = self._traj(x)
        t32 = t_rows.to(device=x.device, dtype=torch.int32).contiguous()
        if t32.numel() != B:
            raise RuntimeError(f"time must have one entry per row: got {t32.numel()} for batch {B}")
        out = torch.empty_like(x)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_unet_forward_rows(
                self._h, x.data_ptr(), t32.data_ptr(), out.data_ptr(), B, ws.data_ptr(),
                ws.numel() * 4, self._stream()))
        return out

    def denoise_step(self, x: torch.Tensor, t: int, *, noise: Optional[torch.Tensor] = None,
                     seed: int = 0, row_offset: int = 0, draw: int = 0,
                     cond0: Optional[torch.Tensor] = None,
                     guide_grad: Optional[torch.Tensor] = None, guide_weight: float = 0.0,
                     mean_out: Optional[torch.Tensor] = None,
                     eps_out: Optional[torch.Tensor] = None, update_x: bool = True) -> None:
        """In-place reverse step on ``x`` (see dad_denoise_step in include/dad.h)."""
        self._step(self.lib.dad_denoise_step, int(t), x, noise, seed, row_offset, draw, cond0, guide_grad,
                   guide_weight, mean_out, eps_out, update_x)

    def sampler_step(self, x: torch.Tensor, coef, *, noise: Optional[torch.Tensor] = None,
                     seed: int = 0, row_offset: int = 0, draw: int = 0,
                     cond0: Optional[torch.Tensor] = None,
                     guide_grad: Optional[torch.Tensor] = None, guide_weight: float = 0.0,
                     mean_out: Optional[torch.Tensor] = None,
                     eps_out: Optional[torch.Tensor] = None, update_x: bool = True) -> None:
        """``denoise_step`` with the step given by its coefficients: ``coef`` is one element of
        ``pack_sampler_steps`` (see dad_sampler_step in include/dad.h)."""
        one = _steps_array(np.asarray(coef).reshape(-1), "coef")
        if one.shape[0] != 1:
            raise ValueError("sampler_step takes one step")
        self._step(self.lib.dad_sampler_step, one.ctypes.data, x, noise, seed, row_offset, draw, cond0, guide_grad,
                   guide_weight, mean_out, eps_out, update_x)

    def _step(self, call, which, x, noise, seed, row_offset, draw, cond0, guide_grad, guide_weight, mean_out,
              eps_out, update_x):
        """One reverse step through ``call``, which takes the step itself (``which``: a timestep or a coefficient
        row) right after ``x``."""
        B = self._traj(x)
        a = DadStepArgs()
        for name, ten in (("noise", noise), ("guide_grad", guide_grad), ("mean_out", mean_out),
                          ("eps_out", eps_out)):
            if ten is not None:
                if self._traj(ten, name) != B:
                    raise RuntimeError(f"{name} batch mismatch")
                setattr(a, name, ten.data_ptr())
        a.seed, a.row_offset, a.draw = int(seed), int(row_offset), int(draw)
        a.cond0, a.cond_per_row = self._cond0(cond0, B)
        a.guide_weight = float(guide_weight)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            _check(self.lib, call(
                self._h, x.data_ptr(), which, B, C.byref(a), int(not update_x), ws.data_ptr(),
                ws.numel() * 4, self._stream()))

    def _cond0(self, cond0: Optional[torch.Tensor], B: int):
        """(pointer, one row per trajectory?) of the horizon-step-0 condition, (1, td) or (B, td)."""
        if cond0 is None:
            return None, 0
        _require_device(cond0, "cond0")
        rows = cond0.reshape(-1, self.transition_dim).shape[0]
        if rows not in (1, B):
            raise RuntimeError(f"cond0 must be (1, td) or (B, td), got {tuple(cond0.shape)}")
        return cond0.data_ptr(), int(rows == B and B > 1)

    def sample_loop(self, x: torch.Tensor, n_steps: int, *,
                    noise_stack: Optional[torch.Tensor] = None, seed: int = 0,
                    row_offset: int = 0, cond0: Optional[torch.Tensor] = None,
                    projection: Optional["ProjectionState"] = None,
                    proj_alphas: Optional[Sequence[float]] = None,
                    use_graph: bool = False, guide: Optional["GuideState"] = None, guide_weight: float = 0.0) -> None:
        """``guide`` (a :class:`GuideState`) with a positive ``guide_weight``: the same loop with the guide evaluated
        inside it (:meth:`guided_loop`)."""
        if guide is not None and guide_weight > 0:
            order = None if projection is None else [float(proj_alphas[t]) for t in reversed(range(int(n_steps)))]
            return self.guided_loop(x, guide, guide_weight, n_steps=int(n_steps), noise_stack=noise_stack, seed=seed,
                                    row_offset=row_offset, cond0=cond0, projection=projection, proj_alphas=order,
                                    use_graph=use_graph)
        alphas = None
        if projection is not None:
            alphas = (C.c_float * self.n_timesteps)(*[float(a) for a in proj_alphas])
        self._loop(self.lib.dad_sample_loop, (int(n_steps),), int(n_steps), x, noise_stack, seed, row_offset, cond0,
                   projection, alphas, use_graph)

    def sampler_loop(self, x: torch.Tensor, steps, *,
                     noise_stack: Optional[torch.Tensor] = None, seed: int = 0,
                     row_offset: int = 0, cond0: Optional[torch.Tensor] = None,
                     projection: Optional["ProjectionState"] = None,
                     proj_alphas: Optional[Sequence[float]] = None,
                     use_graph: bool = False, guide: Optional["GuideState"] = None, guide_weight: float = 0.0) -> None:
        """``sample_loop`` over caller-given steps: ``steps`` is ``pack_sampler_steps`` in execution order, and so are
        ``proj_alphas`` and ``noise_stack`` (see dad_sampler_loop in include/dad.h).  ``guide`` / ``guide_weight`` as
        :meth:`sample_loop`."""
        if guide is not None and guide_weight > 0:
            return self.guided_loop(x, guide, guide_weight, steps=steps, noise_stack=noise_stack, seed=seed,
                                    row_offset=row_offset, cond0=cond0, projection=projection, proj_alphas=proj_alphas,
                                    use_graph=use_graph)
        arr = _steps_array(steps, "steps")
        n_steps = int(arr.shape[0])
        alphas = None
        if projection is not None:
            if proj_alphas is None or len(proj_alphas) != n_steps:
                raise ValueError("proj_alphas must hold one strength per step, in execution order")
            alphas = (C.c_float * n_steps)(*[float(a) for a in proj_alphas])
        self._loop(self.lib.dad_sampler_loop, (arr.ctypes.data, n_steps), n_steps, x, noise_stack, seed, row_offset,
                   cond0, projection, alphas, use_graph)

    def guided_loop(self, x: torch.Tensor, guide: "GuideState", guide_weight: float, *, steps=None,
                    n_steps: Optional[int] = None, noise_stack: Optional[torch.Tensor] = None, seed: int = 0,
                    row_offset: int = 0, cond0: Optional[torch.Tensor] = None,
                    projection: Optional["ProjectionState"] = None,
                    proj_alphas: Optional[Sequence[float]] = None, use_graph: bool = False) -> None:
        """The fused loop with a library guide inside it (see dad_guided_loop in include/dad.h): ``steps`` as
        :meth:`sampler_loop` takes them, or None for the ``n_steps`` ancestral steps of the loaded schedule;
        ``proj_alphas`` in execution order either way.  The gradient scratch the guide launch hands to the step's
        tail is the guide's own, or under ``use_graph`` a persistent buffer of this engine (a frozen pointer)."""
        arr = None
        if steps is not None:
            arr = _steps_array(steps, "steps")
            n_steps = int(arr.shape[0])
        if n_steps is None:
            raise ValueError("guided_loop needs steps or n_steps")
        alphas = None
        if projection is not None:
            if proj_alphas is None or len(proj_alphas) != n_steps:
                raise ValueError("proj_alphas must hold one strength per step, in execution order")
            alphas = (C.c_float * n_steps)(*[float(a) for a in proj_alphas])
        self._traj(x)
        ga = None
        if guide is not None and guide_weight > 0:
            guide.refresh()
            guide.bind_scratch(self.persistent("guide_grad", tuple(x.shape)) if use_graph else None, x)
            ga = C.byref(guide.args)
        self._loop(self.lib.dad_guided_loop, (None if arr is None else arr.ctypes.data, int(n_steps)), int(n_steps), x,
                   noise_stack, seed, row_offset, cond0, projection, alphas, use_graph, (ga, float(guide_weight)))

    def _loop(self, call, which, n_steps, x, noise_stack, seed, row_offset, cond0, projection, alphas, use_graph,
              guide=()):
        """One fused loop through ``call``, which takes the steps themselves (``which``: their number, or their
        coefficients and their number) right after ``x``; ``alphas`` is the C array that call reads; ``guide``: the
        two arguments dad_guided_loop takes after the condition."""
        B = self._traj(x)
        cond_ptr, per_row = self._cond0(cond0, B)
        if noise_stack is not None:
            _require_device(noise_stack, "noise_stack")
            if tuple(noise_stack.shape) != (n_steps, B, self.horizon, self.transition_dim):
                raise RuntimeError("noise_stack must be (n_steps, B, H, td)")
        pa = None
        if projection is not None:
            projection._check_x(x)
            pa = C.byref(projection.args)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            _check(self.lib, call(
                self._h, x.data_ptr(), *which, B, _ptr(noise_stack), int(seed),
                int(row_offset), cond_ptr, per_row, *guide, pa, alphas, int(use_graph), ws.data_ptr(),
                ws.numel() * 4, self._stream()))

    def fill_normal(self, x: torch.Tensor, seed: int, row_offset: int = 0, draw: int = 0) -> None:
        _require_device(x, "x")
        B = int(x.shape[0])
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_fill_normal(
                x.data_ptr(), B, x.numel() // B, int(seed), int(row_offset), int(draw),
                self._stream()))

    # ------------------------------------------------------------------ training
    def refresh(self, unet_state: Mapping[str, torch.Tensor]) -> None:
        """Re-derive the engine's packed copies from parameter tensors that already live on this device
        (fp32, contiguous): no host round trip (dad_model_refresh_weights)."""
        keys, ptrs, keep = [], [], []
        if self.widths_padded:             # the padded tensors are rebuilt on the device: one scatter for all of them
            with torch.no_grad():
                names = list(unet_state.keys())
                fp = self.flat_padding(names, [tuple(unet_state[k].shape) for k in names])
                wide = fp.pad_flat([unet_state[k].detach().to(self.device) for k in names])
            base, n = wide.data_ptr(), len(names)        # (FlatPadding's packed offsets are 16-byte aligned)
            with torch.cuda.device(self.device):
                _check(self.lib, self.lib.dad_model_refresh_weights(
                    self._h, n, (C.c_char_p * n)(*[k.encode() for k in names]),
                    (C.c_void_p * n)(*[base + 4 * o for o in fp.offsets]), self._stream()))
            self._refresh_keep = [wide]
            return
        for key, t in unet_state.items():
            d = t.detach()
            if d.device != self.device or d.dtype != torch.float32 or not d.is_contiguous():
                d = d.to(self.device, torch.float32).contiguous()
            keep.append(d)
            keys.append(key.encode())
            ptrs.append(d.data_ptr())
        n = len(keys)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_model_refresh_weights(
                self._h, n, (C.c_char_p * n)(*keys), (C.c_void_p * n)(*ptrs), self._stream()))
        self._refresh_keep = keep          # (stream-ordered: the copies run before anything enqueued later)

    def flat_padding(self, keys, shapes, offsets=None, total=None):
        """utils/padding.FlatPadding of the named tensors (real shapes) for this net's zero-padded widths."""
        from .utils import padding
        cache = self.__dict__.setdefault("_flat_paddings", {})
        sig = (tuple(keys), None if offsets is None else tuple(offsets))
        if sig not in cache:
            cache[sig] = padding.FlatPadding(keys, shapes, self._pad_plan, offsets, total)
        return cache[sig]

    def time_projection_index(self) -> torch.Tensor:
        """Column of every real time-projection entry in the padded rows the training forward reads: the blocks'
        projections side by side in launch order, each at its level's padded width."""
        from .utils import padding
        cached = getattr(self, "_temb_index", None)
        if cached is None:
            n = len(self.real_channels)
            widths = [c for c in self.real_channels for _ in (0, 1)] + [self.real_channels[-1]] * 2
            for j in range(n - 1):
                widths += [self.real_channels[n - 2 - j]] * 2
            index, off = [], 0
            for c in widths:
                index.append(padding.channel_index(c) + off)
                off += padding.padded_width(c)
            cached = self._temb_index = (torch.cat(index).to(self.device), off)
        return cached

    def grad_layout(self):
        """[(reference key without 'model.', offset in floats, numel)] of the flat gradient buffer and
        its total length."""
        cached = getattr(self, "_grad_layout", None)      # (a property of the architecture: asked once)
        if cached is not None:
            return cached
        n, total = C.c_int32(), C.c_int64()
        _check(self.lib, self.lib.dad_train_grad_count(self._h, C.byref(n), C.byref(total)))
        out = []
        for i in range(n.value):
            key, off, numel = C.c_char_p(), C.c_int64(), C.c_int64()
            _check(self.lib, self.lib.dad_train_grad_info(self._h, i, C.byref(key), C.byref(off), C.byref(numel)))
            out.append((key.value.decode(), off.value, numel.value))
        self._grad_layout = (out, total.value)
        return self._grad_layout

    def train_forward(self, x: torch.Tensor, temb_rows: torch.Tensor):
        """eps_theta(x) with per-row time projections ``temb_rows`` (B, temb_width), keeping every
        activation: returns (out, saved) — ``saved`` goes to :meth:`train_backward`."""
        B = self._traj(x)
        _require_device(temb_rows, "temb_rows")
        if temb_rows.dim() != 2 or temb_rows.shape[0] != B:
            raise RuntimeError(f"temb_rows must be (B, temb_width), got {tuple(temb_rows.shape)}")
        sv, sc = C.c_size_t(), C.c_size_t()
        _check(self.lib, self.lib.dad_train_workspace_bytes(self._h, B, C.byref(sv), C.byref(sc)))
        saved = torch.empty(max(sv.value, 4) // 4 + 4, dtype=torch.float32, device=self.device)
        rows = torch.arange(B, dtype=torch.int32, device=self.device)
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_unet_forward_train(
                self._h, x.data_ptr(), rows.data_ptr(), temb_rows.data_ptr(), out.data_ptr(), B,
                saved.data_ptr(), saved.numel() * 4, self._stream()))
        return out, saved

    def train_backward(self, x: torch.Tensor, d_out: torch.Tensor, saved: torch.Tensor, temb_width: int, shapes):
        """(d_x, d_temb_rows, [one gradient tensor per entry of grad_layout(), shaped like ``shapes``]) for
        one batch (see dad_unet_backward).  Separate tensors: autograd adopts them as ``.grad`` without copying."""
        B = self._traj(x)
        if self._traj(d_out, "d_out") != B:
            raise RuntimeError("d_out batch mismatch")
        sv, sc = C.c_size_t(), C.c_size_t()
        _check(self.lib, self.lib.dad_train_workspace_bytes(self._h, B, C.byref(sv), C.byref(sc)))
        scratch = torch.empty(max(sc.value, 4) // 4 + 4, dtype=torch.float32, device=self.device)
        layout, total = self.grad_layout()
        if len(shapes) != len(layout):
            raise RuntimeError(f"{len(shapes)} parameter shapes for {len(layout)} gradient tensors")
        real = None
        if self.widths_padded:
            # zero-padded widths: the library fills padded gradients; `shapes` are the REAL parameters' — one gather
            # over the flat buffer picks the real entries (utils/padding.FlatPadding), the padding's are dropped
            real = self.flat_padding([k for k, _, _ in layout], shapes, [o for _, o, _ in layout], total)
            shapes = real.padded_shapes
            for (key, _, numel), n in zip(layout, real.sizes):
                if n != numel:
                    raise RuntimeError(f"{key}: {n} padded elements, the library expects {numel}")
        # ONE allocation per step, split into per-parameter views at the library's own (16-byte aligned) offsets:
        # autograd adopts a contiguous view as `.grad` as it does a tensor of its own (no copy), and the host side of
        # a step loses ~150 allocator calls
        flat = torch.empty(total, dtype=torch.float32, device=self.device)
        base = flat.data_ptr()
        spans = [layout[i + 1][1] - layout[i][1] for i in range(len(layout) - 1)] + [total - layout[-1][1]]
        pieces = flat.split_with_sizes(spans)              # one call: a view per slot (slots are padded to 4 floats)
        grads = [(pc if pc.numel() == numel else pc[:numel]).view(tuple(shape))
                 for pc, (_, _, numel), shape in zip(pieces, layout, shapes)]
        ptrs = (C.c_void_p * len(grads))(*[base + 4 * offset for _, offset, _ in layout])
        d_x = torch.empty_like(x)
        d_temb = torch.empty(B, temb_width, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_unet_backward(
                self._h, x.data_ptr(), d_out.data_ptr(), d_x.data_ptr(), d_temb.data_ptr(), ptrs, len(grads), B,
                saved.data_ptr(), saved.numel() * 4, scratch.data_ptr(), scratch.numel() * 4, self._stream()))
        if real is not None:
            grads = real.gather(flat)
        return d_x, d_temb, grads

    # ------------------------------------------------------------------ fused training objective
    def bind_train_schedule(self, sqrt_ac: torch.Tensor, sqrt_1m_ac: torch.Tensor) -> None:
        """Hand over the two schedule vectors q_sample reads (dad_model_load_train_schedule); a no-op while the
        same buffers are bound."""
        sig = (sqrt_ac.data_ptr(), sqrt_ac._version, sqrt_1m_ac.data_ptr(), sqrt_1m_ac._version)
        if getattr(self, "_train_sched_sig", None) == sig:
            return
        a = sqrt_ac.detach().to("cpu", torch.float32).contiguous()
        b = sqrt_1m_ac.detach().to("cpu", torch.float32).contiguous()
        if a.numel() != self.n_timesteps or b.numel() != self.n_timesteps:
            raise ValueError(f"training schedule has {a.numel()} / {b.numel()} entries, expected {self.n_timesteps}")
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_model_load_train_schedule(self._h, a.data_ptr(), b.data_ptr(), self.n_timesteps))
        self._train_sched_sig = sig

    def time_grad_layout(self):
        """[(time-MLP key, offset in floats, numel)] of the time gradients' own flat buffer and its length."""
        cached = getattr(self, "_time_grad_layout", None)
        if cached is not None:
            return cached
        n, total = C.c_int32(), C.c_int64()
        _check(self.lib, self.lib.dad_train_time_grad_count(self._h, C.byref(n), C.byref(total)))
        out = []
        for i in range(n.value):
            key, off, numel = C.c_char_p(), C.c_int64(), C.c_int64()
            _check(self.lib, self.lib.dad_train_time_grad_info(self._h, i, C.byref(key), C.byref(off), C.byref(numel)))
            out.append((key.value.decode(), off.value, numel.value))
        self._time_grad_layout = (out, total.value)
        return self._time_grad_layout

    def _objective_bytes(self, batch: int):
        """(saved, scratch) bytes of an objective step at `batch`: asked once per batch size (the debug hooks, which
        change the plan, drop the answers)."""
        cache = self.__dict__.setdefault("_objective_sizes", {})
        if batch not in cache:
            sv, sc = C.c_size_t(), C.c_size_t()
            _check(self.lib, self.lib.dad_train_objective_workspace_bytes(self._h, batch, C.byref(sv), C.byref(sc)))
            cache[batch] = (sv.value, sc.value)
        return cache[batch]

    def objective_forward(self, x0: torch.Tensor, t32: torch.Tensor, noise: torch.Tensor,
                          weights: Optional[torch.Tensor], loss_type: int):
        """The training objective of one batch (dad_train_objective_forward): returns (loss, saved) — a device
        scalar and what :meth:`objective_backward` needs.  ``t32``: (B) int32 on the device."""
        B = self._traj(x0, "x_start")
        for name, ten in (("noise", noise), ("weights", weights)):
            if ten is not None and self._traj(ten, name) != B:
                raise RuntimeError(f"{name} batch mismatch")
        if t32.dtype != torch.int32 or t32.numel() != B or t32.device != x0.device or not t32.is_contiguous():
            raise RuntimeError("t must be (B) contiguous int32 on the trajectory's device")
        sv, _ = self._objective_bytes(B)
        saved = torch.empty(max(sv, 4) // 4 + 4, dtype=torch.float32, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_train_objective_forward(
                self._h, x0.data_ptr(), t32.data_ptr(), noise.data_ptr(), _ptr(weights), int(loss_type),
                loss.data_ptr(), B, saved.data_ptr(), saved.numel() * 4, self._stream()))
        return loss, saved

    def objective_backward(self, x0: torch.Tensor, noise: torch.Tensor, weights: Optional[torch.Tensor],
                           loss_type: int, d_loss: torch.Tensor, saved: torch.Tensor, shapes):
        """Every parameter gradient of one batch (dad_train_objective_backward): the tensors of grad_layout() followed
        by those of time_grad_layout(), shaped like ``shapes`` (the real parameters'), all views of ONE flat allocation.
        ``d_loss``: autograd's incoming scalar, on the device; it is read there."""
        B = self._traj(x0, "x_start")
        _require_device(d_loss, "d_loss")
        _, sc = self._objective_bytes(B)
        scratch = torch.empty(max(sc, 4) // 4 + 4, dtype=torch.float32, device=self.device)
        flat, ptrs, tptrs, finish = self._grad_buffers(shapes)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_train_objective_backward(
                self._h, x0.data_ptr(), noise.data_ptr(), _ptr(weights), int(loss_type), d_loss.data_ptr(),
                ptrs, len(ptrs), tptrs, len(tptrs), B, saved.data_ptr(), saved.numel() * 4,
                scratch.data_ptr(), scratch.numel() * 4, self._stream()))
        return finish(flat)

    def _grad_buffers(self, shapes):
        """The flat gradient allocation of one objective backward: (flat, conv pointers, time pointers, finish), where
        ``finish(flat)`` returns the tensors shaped like ``shapes`` (as :meth:`objective_backward` returns them)."""
        conv, conv_total = self.grad_layout()
        time, time_total = self.time_grad_layout()
        layout = list(conv) + [(k, conv_total + o, n) for k, o, n in time]
        total = conv_total + time_total
        if len(shapes) != len(layout):
            raise RuntimeError(f"{len(shapes)} parameter shapes for {len(layout)} gradient tensors")
        real = None
        if self.widths_padded:             # (as train_backward: the library fills padded gradients, one gather picks the real entries)
            real = self.flat_padding([k for k, _, _ in layout], shapes, [o for _, o, _ in layout], total)
            shapes = real.padded_shapes
            for (key, _, numel), n in zip(layout, real.sizes):
                if n != numel:
                    raise RuntimeError(f"{key}: {n} padded elements, the library expects {numel}")
        flat = torch.empty(total, dtype=torch.float32, device=self.device)
        base = flat.data_ptr()
        ptrs = (C.c_void_p * len(conv))(*[base + 4 * o for _, o, _ in layout[:len(conv)]])
        tptrs = (C.c_void_p * len(time))(*[base + 4 * o for _, o, _ in layout[len(conv):]])

        def finish(flat):
            if real is not None:
                return real.gather(flat)
            spans = [layout[i + 1][1] - layout[i][1] for i in range(len(layout) - 1)] + [total - layout[-1][1]]
            return [(pc if pc.numel() == numel else pc[:numel]).view(tuple(shape))
                    for pc, (_, _, numel), shape in zip(flat.split_with_sizes(spans), layout, shapes)]
        return flat, ptrs, tptrs, finish

    # ------------------------------------------------------------------ dynamics-aware objective
    def _dynamics_bytes(self, state: "ProjectionState", form: int, batch: int):
        """(saved, scratch) bytes of a dynamics-aware objective step (dad_train_dynamics_objective_workspace_bytes)."""
        a = state.args
        key = ("dyn", a.state_dim, a.observation_dim, a.action_dim, form, batch)
        cache = self.__dict__.setdefault("_objective_sizes", {})
        if key not in cache:
            sv, sc = C.c_size_t(), C.c_size_t()
            _check(self.lib, self.lib.dad_train_dynamics_objective_workspace_bytes(self._h, C.byref(a), form, batch,
                                                                                   C.byref(sv), C.byref(sc)))
            cache[key] = (sv.value, sc.value)
        return cache[key]

    def dynamics_objective_forward(self, x0: torch.Tensor, t32: torch.Tensor, noise: torch.Tensor,
                                   weights: Optional[torch.Tensor], loss_type: int, state: "ProjectionState", form: int,
                                   diffusion_weight: float, projection_weight: float,
                                   timestep_weights: Optional[torch.Tensor]):
        """The dynamics-aware objective of one batch (dad_train_dynamics_objective_forward): returns (parts, saved) —
        the device float[3] (diffusion, weighted projection, total) and what :meth:`dynamics_objective_backward` needs."""
        B = self._traj(x0, "x_start")
        for name, ten in (("noise", noise), ("weights", weights)):
            if ten is not None and self._traj(ten, name) != B:
                raise RuntimeError(f"{name} batch mismatch")
        if t32.dtype != torch.int32 or t32.numel() != B or t32.device != x0.device or not t32.is_contiguous():
            raise RuntimeError("t must be (B) contiguous int32 on the trajectory's device")
        if timestep_weights is not None:
            _require_device(timestep_weights, "timestep_weights")
            if timestep_weights.numel() != self.n_timesteps:
                raise RuntimeError(f"timestep_weights has {timestep_weights.numel()} entries, expected {self.n_timesteps}")
        if state.P.device != x0.device:
            raise RuntimeError(f"x is on {x0.device}, the projector on {state.P.device}")
        sv, _ = self._dynamics_bytes(state, form, B)
        saved = torch.empty(max(sv, 4) // 4 + 4, dtype=torch.float32, device=self.device)
        parts = torch.empty(3, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_train_dynamics_objective_forward(
                self._h, x0.data_ptr(), t32.data_ptr(), noise.data_ptr(), _ptr(weights), int(loss_type),
                C.byref(state.args), int(state.D), int(form), float(diffusion_weight), float(projection_weight),
                _ptr(timestep_weights), parts.data_ptr(), B, saved.data_ptr(), saved.numel() * 4, self._stream()))
        return parts, saved

    def dynamics_objective_backward(self, x0: torch.Tensor, noise: torch.Tensor, weights: Optional[torch.Tensor],
                                    loss_type: int, state: "ProjectionState", form: int, diffusion_weight: float,
                                    projection_weight: float, timestep_weights: Optional[torch.Tensor],
                                    d_loss: torch.Tensor, saved: torch.Tensor, shapes):
        """Every parameter gradient of the total (dad_train_dynamics_objective_backward), as :meth:`objective_backward`
        returns them.  ``d_loss``: autograd's incoming scalar, on the device; it is read there."""
        B = self._traj(x0, "x_start")
        _require_device(d_loss, "d_loss")
        _, sc = self._dynamics_bytes(state, form, B)
        scratch = torch.empty(max(sc, 4) // 4 + 4, dtype=torch.float32, device=self.device)
        flat, ptrs, tptrs, finish = self._grad_buffers(shapes)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_train_dynamics_objective_backward(
                self._h, x0.data_ptr(), noise.data_ptr(), _ptr(weights), int(loss_type), C.byref(state.args), int(state.D),
                int(form), float(diffusion_weight), float(projection_weight), _ptr(timestep_weights), d_loss.data_ptr(),
                ptrs, len(ptrs), tptrs, len(tptrs), B, saved.data_ptr(), saved.numel() * 4,
                scratch.data_ptr(), scratch.numel() * 4, self._stream()))
        return finish(flat)

    def dynamics_objective_plan(self, batch: int, state_dim: int = None, observation_dim: int = None, action_dim: int = None,
                                form: Optional[str] = None, *, state: "ProjectionState" = None) -> dict:
        """What one dynamics-aware objective step adds to the fused objective's (:meth:`objective_plan`) at `batch`, for a
        projector over these widths (or ``state``'s) under ``form`` (None: planned, "row", "gemm"): host logic only
        (dad_debug_dynamics_objective_plan).  Keys as DAD_DO_* of include/dad.h: ``form`` ("row" / "gemm"), ``D``,
        ``horizon``, ``col_blocks``, ``refused``, the layout (``saved_base``, ``saved_bytes``, ``scratch_base``,
        ``scratch_bytes`` in bytes; ``r_offset``, ``part_offset``, ``violation_offset``, ``g_offset`` in floats behind the
        bases), ``objective_launches``, ``fwd_launches`` and ``launches``: one dict per launch of the step's own kernels,
        the forward's first, with ``kind`` (a name of DAD_DO_KINDS), ``grid`` (x, y), ``threads``, ``lds_bytes`` and
        ``rows_per_block``."""
        if state is not None:
            state_dim, observation_dim, action_dim = state.args.state_dim, state.args.observation_dim, state.args.action_dim
        head, launches = decode_report(
            _fetch(self.lib.dad_debug_dynamics_objective_plan, self._h, int(batch), int(state_dim), int(observation_dim),
                   int(action_dim), _violation_form(form)), "DAD_DO_HEADER", "DAD_DO_REC_INTS")
        assert head["launches"] == len(launches)
        kinds = _names("DAD_DO_KINDS")
        for q in launches:
            q["kind"] = kinds[q["kind"]]
            q["grid"] = (q.pop("gx"), q.pop("gy"))
        head["form"], head["refused"] = _names("DAD_VG_FORMS")[head["form"]], bool(head["refused"])
        head["launches"] = launches
        return head

    def objective_saved_views(self, saved: torch.Tensor, batch: int):
        """(x_t, denoiser output) as the last objective_forward left them in ``saved`` (test hook)."""
        a, b = C.c_size_t(), C.c_size_t()
        _check(self.lib, self.lib.dad_debug_objective_offsets(self._h, int(batch), C.byref(a), C.byref(b)))
        n = batch * self.horizon * self.transition_dim
        shape = (batch, self.horizon, self.transition_dim)
        return saved[a.value // 4:a.value // 4 + n].view(shape), saved[b.value // 4:b.value // 4 + n].view(shape)

    # ------------------------------------------------------------------ test / tuning hooks
    def debug_set_tile(self, cfg: int) -> None:
        """Force a conv tile (0..9), -1 = heuristic, 100+cfg / 99 = same without grid split-K."""
        self.__dict__.pop("_objective_sizes", None)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_debug_set_tile(self._h, int(cfg)))

    def debug_set_option(self, name: str, value: int) -> None:
        # (the entry point synchronises the CURRENT device before dropping captured loops)
        self.__dict__.pop("_objective_sizes", None)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_debug_set_option(self._h, name.encode(), int(value)))

    def read_table(self, which: str, t: int) -> torch.Tensor:
        """Row t of a per-timestep table (see DAD_TABLE_* in include/dad.h), as a CPU tensor."""
        out = torch.empty(1 << 16, dtype=torch.float32)
        width = C.c_int32()
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_debug_read_table(self._h, TABLES[which], int(t),
                                                           out.data_ptr(), out.numel(), C.byref(width)))
        return out[:width.value].clone()

    def seam_plan(self, batch: int, *, projection: bool = False, detail: bool = False) -> dict:
        """Whether dad_sample_loop at `batch` (``projection``: with a projection argument) runs the seam between two
        denoise steps as one launch (csrc/conv_seam.hpp) under the current debug options (dad_debug_seam_plan: the
        statement the loop itself reads; host logic only).  Returns ``taken``, ``reason`` (the name of the first
        condition that refuses it, "taken" otherwise), ``grid``, ``threads``, ``lds_bytes``, ``tile`` (the first conv's
        tile, whose summation order the launch keeps) and ``units`` (8-channel units multiplied).  With ``detail`` also
        the fields that name the path inside the kernel: ``spt`` (samples of a 32-row tile), ``last`` (samples in the
        last tile), ``buffers`` (which allowed relation final_act has to the buffers the launch writes: "apart", "dst"
        or "rdst"; None when refused) and ``dim`` / ``tile0``: the instantiation conv_seam_f32<dim, tile0>."""
        out = (C.c_int32 * _fields("DAD_SEAM_INTS")[1])()
        _check(self.lib, self.lib.dad_debug_seam_plan(self._h, int(batch), int(bool(projection)), out))
        q = _decode("DAD_SEAM_INTS", out)
        q["taken"], q["reason"] = bool(q["taken"]), self.lib.dad_debug_seam_reason(q["reason"]).decode()
        q["buffers"] = _names("DAD_SEAM_BUFS")[q["buffers"]] if q["buffers"] >= 0 else None
        if not detail:                     # the fields from ``spt`` on name the path inside the kernel
            for k in list(q)[list(q).index("spt"):]:
                del q[k]
        return q

    def halo8_plan(self, batch: int, mode: int = 0) -> list:
        """The conv_halo8_f32 launches (csrc/conv_halo8.hpp) of one evaluation at `batch` under the current debug
        options (dad_debug_halo8_plan: host logic only; ``mode`` 0 / 1 as :meth:`forward_plan`): one dict per launch in
        launch order with the fields of DAD_H8_* — what the kernel makes of the operands the launch hands it."""
        head, recs = decode_report(_fetch(self.lib.dad_debug_halo8_plan, self._h, int(batch), int(mode)), "DAD_H8_HEADER", "DAD_H8_INTS")
        assert head["records"] == len(recs)
        return recs

    def small_batch_plan(self, batch: int):
        """(conv launches through the consumer-combine kernels, how many of them are the
        streamed-weight form for wide layers); (0, 0) when the batch takes the batch-256 kernels."""
        n, w = C.c_int32(), C.c_int32()
        _check(self.lib, self.lib.dad_debug_small_batch_plan(self._h, int(batch), C.byref(n), C.byref(w)))
        return n.value, w.value

    def backward_plan(self, batch: int) -> dict:
        """Which kernels one training step takes at `batch` under the current debug options (host logic only: needs
        ``training=True`` but neither weights nor a device).  Keys as DAD_BP_* of include/dad.h: ``wgrads``, ``multi``
        (launches whose fullest block stages more than one chunk), ``max_chunks``, ``max_ksplit``, ``part``,
        ``part_multi``, ``windowed``, ``tile`` [4], ``taps_tile`` {(taps, tile): launches}, ``fwd`` / ``dgrad``
        {(conv tile cfg, grid split-K?): launches}, and ``launches``: one dict per weight-gradient launch."""
        q, recs = decode_report(_fetch(self.lib.dad_debug_backward_plan, self._h, int(batch)), "DAD_BP_HEADER", "DAD_BP_REC_INTS")
        assert q["wgrads"] == len(recs)
        tiles = len(q["tile"])
        q["taps_tile"] = {(taps, tile): n for i, taps in enumerate((1, 3, 4, 5, 7)) for tile in range(tiles)
                          if (n := q["taps_tile"][tiles * i + tile])}
        for name in ("fwd", "dgrad"):      # launches per (conv tile cfg, grid split-K?)
            q[name] = {(i // 2, bool(i % 2)): n for i, n in enumerate(q[name]) if n}
        q["launches"] = recs
        return q

    def backward_steps(self, batch: int) -> dict:
        """Everything dad_unet_backward replays at `batch` under the current debug options (dad_debug_backward_steps:
        host logic only, as :meth:`backward_plan`).  Returns ``batch``, ``colsums`` (launches, entries, widest),
        ``padcopy`` (the zero-padded horizon's copies run), ``horizon`` / ``real_horizon``, ``dx`` and ``steps``: one
        dict per step in launch order with ``kind`` ("bias", "wgrad", "dgrad", "gn", "resid" or "cols": DAD_BS_K_* of
        include/dad.h) and the fields that kind's list there names (DAD_BS_*_INTS_LIST); ``write`` is a name of BS_WRITES."""
        kinds, ints = _names("DAD_BS_KINDS"), _fetch(self.lib.dad_debug_backward_steps, self._h, int(batch))
        head, steps = decode_report(ints, "DAD_BS_HEADER",      # a kind's list is named after it: DAD_BS_WGRAD_INTS
                                    lambda head, at: f"DAD_BS_{kinds[_decode('DAD_BS_REC_INTS', ints, at)['kind']].upper()}_INTS")
        assert head["steps"] == len(steps)
        for q in steps:
            q["kind"] = kinds[q.pop("kind")]
            if "write" in q:
                q["write"] = BS_WRITES[q["write"]]
        return {"batch": head["batch"], "colsums": (head["colsums_launches"], head["colsums_entries"], head["colsums_widest"]),
                "padcopy": bool(head["padcopy"]), "horizon": head["horizon"], "real_horizon": head["real_horizon"],
                "dx": bool(head["dx"]), "steps": steps}

    def objective_plan(self, batch: int) -> dict:
        """The time chain of one fused objective step at `batch` (host logic only, as :meth:`backward_plan`).  Keys as
        DAD_OP_* of include/dad.h: ``loss_blocks``, ``kslices``, ``kslice``, ``temb_width``, ``blocks``, ``n``, and
        ``launches``: one dict per launch in launch order with ``mode`` (a name of TIME_GEMM_MODES), ``M``, ``N``,
        ``K``, ``grid`` (x, y, z), ``chunks`` (32-wide K chunks of a full slice), ``last_chunks``, ``ktail`` (K % 32)
        and ``kslice``."""
        head, launches = decode_report(_fetch(self.lib.dad_debug_objective_plan, self._h, int(batch)), "DAD_OP_HEADER", "DAD_OP_REC_INTS")
        assert head["launches"] == len(launches)
        modes = _names("DAD_OP_TG_MODES")
        for q in launches:
            q["mode"] = modes[q["mode"]]
            q["grid"] = (q.pop("gx"), q.pop("gy"), q.pop("gz"))
        head["launches"] = launches
        return head

    def forward_plan(self, batch: int, mode: int = 0) -> dict:
        """What one evaluation launches at `batch` under the current debug options (dad_debug_forward_plan: host logic
        only, needs neither weights nor a device).  ``mode``: 0 the shared-timestep forward (may take the small-batch
        kernels), 1 the same on the batch kernels (per-row timesteps), 2 the training forward, 3 the data-gradient
        convs of the backward pass (2 / 3 need ``training=True``).  Returns ``mode``, ``batch``, ``small`` (the
        small-batch plan is taken), ``final`` (grid x, grid y, kernel name or None) and ``launches``: one dict per
        launch with the fields of DAD_FP_REC_* (``flags``: the flag word of kernel_registered_f) or, with ``small``,
        of DAD_FP_CC_*; each has ``key``, the instantiation it runs: ("gemm", cfg, taps, stride, flags),
        ("halo8", cfg, ride) — conv_halo8_f32 on tile cfg, or with ``wreg`` true its register-weight form
        conv_halo8w_f32 (option "halo8_wreg") —, ("cc", taps, stride, ride, big, rows, windowed) or
        ("ccw", taps, stride, ride, ride_in, rows)."""
        head, launches = decode_report(_fetch(self.lib.dad_debug_forward_plan, self._h, int(batch), int(mode)), "DAD_FP_HEADER",
                                       lambda head, at: "DAD_FP_CC_INTS" if head["small"] else "DAD_FP_REC_INTS")
        assert head["records"] == len(launches)
        small, families = bool(head["small"]), _names("DAD_FP_FAMILIES")
        for q in launches:
            if not small and families[q["family"]] in ("halo8", "halo8w"):
                q["key"] = ("halo8", q["cfg"], (q["flags"] >> FP_FLAGS.index("res")) & 1)
                q["wreg"] = families[q["family"]] == "halo8w"
            elif not small:
                q["key"] = ("gemm", q["cfg"], q["taps"], q["stride"], q["flags"])
            elif q["wide"]:
                q["key"] = ("ccw", q["taps"], q["stride"], q["ride"], q["ride_in"], q["tile_rows"])
            else:
                q["key"] = ("cc", q["taps"], q["stride"], q["ride"], q["big"], q["tile_rows"], q["windowed"])
        final = _names("DAD_FP_FINALS")[head["final_kernel"]]
        return {"mode": head["mode"], "batch": head["batch"], "small": small,
                "final": (head["final_gx"], head["final_gy"], None if final == "none" else final), "launches": launches}

    def mish(self, x: torch.Tensor) -> torch.Tensor:
        """The conv epilogue's Mish applied to a device tensor (test hook)."""
        _require_device(x, "x")
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _check(self.lib, self.lib.dad_debug_mish(x.data_ptr(), out.data_ptr(), x.numel(),
                                                     self._stream()))
        return out

    # ------------------------------------------------------------------ profiling
    def profile_enable(self, on: bool) -> None:
        _check(self.lib, self.lib.dad_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        _check(self.lib, self.lib.dad_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(fl)))
        return ms.value, n.value, fl.value


class _WorkspaceToken:
    """Alive as long as the autograd node that may still read a violation-gradient workspace."""
    __slots__ = ("__weakref__",)


class _ViolationFn(torch.autograd.Function):
    """ProjectionState.violation_fn: dad_projection_violation_fwd keeps the residual in the workspace,
    dad_projection_violation_bwd turns it and d L / d violation into d L / d x."""

    @staticmethod
    def forward(ctx, x, state, form):
        xc = x.detach().contiguous().float()
        state._check_x(xc)
        batch, horizon = int(xc.shape[0]), int(xc.shape[1])
        ws, token = state._grad_workspace(batch, horizon, form)
        out = torch.empty(batch, dtype=torch.float32, device=xc.device)
        lib = load_library()
        with torch.cuda.device(state.device):
            _check(lib, lib.dad_projection_violation_fwd(C.byref(state.args), xc.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                         ws.numel() * 4, batch, horizon, form,
                                                         torch.cuda.current_stream(state.device).cuda_stream))
        ctx.state, ctx.form, ctx.ws, ctx.token = state, form, ws, token
        ctx.x_shape, ctx.x_dtype = tuple(x.shape), x.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_violation):
        state, ws = ctx.state, ctx.ws
        batch, horizon = ctx.x_shape[0], ctx.x_shape[1]
        w = d_violation.contiguous().float()
        d_x = torch.empty(ctx.x_shape, dtype=torch.float32, device=w.device)
        lib = load_library()
        with torch.cuda.device(state.device):
            _check(lib, lib.dad_projection_violation_bwd(C.byref(state.args), w.data_ptr(), d_x.data_ptr(), ws.data_ptr(),
                                                         ws.numel() * 4, batch, horizon, ctx.form,
                                                         torch.cuda.current_stream(state.device).cuda_stream))
        return d_x.to(ctx.x_dtype), None, None


class ProjectionState:
    """Device-resident projector + normaliser statistics for dad_project."""

    def __init__(self, P: torch.Tensor, obs_mean, obs_std, act_mean, act_std, state_dim: int,
                 observation_dim: int, action_dim: int, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("projection kernel needs a ROCm device; there is no CPU path")

        def put(v):
            return torch.as_tensor(v, dtype=torch.float32).contiguous().to(dev)

        self.P = put(P)
        self.obs_mean, self.obs_std = put(obs_mean), put(obs_std)
        self.act_mean, self.act_std = put(act_mean), put(act_std)
        a = DadProjectArgs()
        a.P = self.P.data_ptr()
        a.obs_mean, a.obs_std = self.obs_mean.data_ptr(), self.obs_std.data_ptr()
        a.act_mean, a.act_std = self.act_mean.data_ptr(), self.act_std.data_ptr()
        a.state_dim, a.observation_dim, a.action_dim = state_dim, observation_dim, action_dim
        self.args = a
        self.device = dev
        self._scratch = None
        self.gemm = True          # batches of 32+ trajectories: v @ P as an MFMA GEMM (needs the scratch copy)
        self.D = int(self.P.shape[0])
        if self.P.dim() != 2 or self.P.shape[1] != self.D:
            raise ValueError(f"projection matrix must be square, got {tuple(self.P.shape)}")
        if self.obs_mean.numel() != observation_dim or self.obs_std.numel() != observation_dim \
                or self.act_mean.numel() != action_dim or self.act_std.numel() != action_dim:
            raise ValueError("normaliser statistics do not match observation_dim / action_dim")

    @classmethod
    def host(cls, state_dim: int, observation_dim: int, action_dim: int, gemm: bool = True) -> "ProjectionState":
        """A state without a projector or a device: enough for :meth:`plan` (as an engine without weights plans)."""
        self = cls.__new__(cls)
        self.args = DadProjectArgs()
        self.args.state_dim, self.args.observation_dim, self.args.action_dim = state_dim, observation_dim, action_dim
        self.device, self._scratch, self.gemm, self.D = None, None, gemm, None
        return self

    def _check_x(self, x: torch.Tensor) -> None:
        """The kernel derives D = (H+1) n + H m from x's horizon and indexes P[D, D] with it: a batch
        with another horizon or transition width would read P out of bounds (the reference raises a
        matmul shape error, guides/policies.py:451, losses/__init__.py:181)."""
        _require_device(x, "x")
        a = self.args
        if x.dim() != 3 or x.shape[2] != a.observation_dim + a.action_dim:
            raise RuntimeError(f"x must be (B, H, {a.observation_dim + a.action_dim}), got {tuple(x.shape)}")
        D = (int(x.shape[1]) + 1) * a.state_dim + int(x.shape[1]) * a.action_dim
        if D != self.D:
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({x.shape[0]}x{D} and "
                               f"{self.D}x{self.D}): the projector was built for another horizon")
        if x.device != self.P.device:
            raise RuntimeError(f"x is on {x.device}, the projector on {self.P.device}")
        # scratch copy of the batch for the GEMM form (grown on demand; stable address while the batch
        # size repeats, so captured loops keep their pointer)
        if self.gemm and (self._scratch is None or self._scratch.numel() < x.numel()):
            self._scratch = torch.empty(x.numel(), dtype=torch.float32, device=self.device)
            self.args.scratch = self._scratch.data_ptr()
            self.args.scratch_bytes = self._scratch.numel() * 4

    def plan(self, batch: int, horizon: int, violation: bool = False) -> dict:
        """What :meth:`apply` (or, ``violation``, :meth:`violation`) launches for ``batch`` trajectories of ``horizon``
        steps, with the scratch copy this state would hold for them (:func:`projection_plan`; no device call)."""
        a = self.args
        x_bytes = int(batch) * int(horizon) * (a.observation_dim + a.action_dim) * 4
        scratch = int(a.scratch_bytes) if a.scratch else 0
        if self.gemm:
            scratch = max(scratch, x_bytes)
        return projection_plan(a.state_dim, a.observation_dim, a.action_dim, batch, horizon, scratch_bytes=scratch,
                               violation=violation)

    def violation(self, x: torch.Tensor) -> torch.Tensor:
        """Per-row squared distance from the dynamics-consistent subspace, physical units
        (ProjectionLoss.compute, losses/__init__.py:161-186, before its mean)."""
        self._check_x(x)
        out = torch.empty(int(x.shape[0]), dtype=torch.float32, device=x.device)
        lib = load_library()
        with torch.cuda.device(self.device):
            _check(lib, lib.dad_projection_violation(C.byref(self.args), x.data_ptr(), out.data_ptr(),
                                                     int(x.shape[0]), int(x.shape[1]),
                                                     torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def grad_plan(self, batch: int, horizon: int, form: Optional[str] = None) -> dict:
        """What :meth:`violation_fn` launches, forward and backward, for ``batch`` trajectories of ``horizon`` steps
        under ``form`` (:func:`violation_grad_plan`; no device call)."""
        a = self.args
        return violation_grad_plan(a.state_dim, a.observation_dim, a.action_dim, batch, horizon, form)

    def _grad_workspace(self, batch: int, horizon: int, form: int):
        """(workspace, token) for one forward / backward pair.  The state keeps one workspace, grown on demand; the
        token lives on the autograd node, and while the node of an earlier call is alive (its backward may still
        come) a later call gets a workspace of its own instead of overwriting the residual that backward needs."""
        lib, need = load_library(), C.c_size_t()
        _check(lib, lib.dad_violation_grad_workspace_bytes(C.byref(self.args), batch, horizon, form, C.byref(need)))
        floats = (need.value + 3) // 4
        holder = getattr(self, "_vg_holder", None)
        token = _WorkspaceToken()
        if holder is not None and holder() is not None:
            return torch.empty(floats, dtype=torch.float32, device=self.device), token
        ws = getattr(self, "_vg_ws", None)
        if ws is None or ws.numel() < floats:
            ws = self._vg_ws = torch.empty(floats, dtype=torch.float32, device=self.device)
        self._vg_holder = weakref.ref(token)
        return ws, token

    def violation_fn(self, x: torch.Tensor, form: Optional[str] = None) -> torch.Tensor:
        """:meth:`violation` with a graph to ``x``: the per-row violation (B,) as one autograd node whose backward is
        dad_projection_violation_bwd (once differentiable; the projector gets no gradient, as in the reference, where
        it is a plain tensor).  ``form``: None lets the planner choose, "row" / "gemm" force a form (a test hook)."""
        return _ViolationFn.apply(x, self, _violation_form(form))

    def apply(self, x: torch.Tensor, alpha: float) -> None:
        self._check_x(x)
        lib = load_library()
        with torch.cuda.device(self.device):
            _check(lib, lib.dad_project(C.byref(self.args), float(alpha), x.data_ptr(),
                                        int(x.shape[0]), int(x.shape[1]),
                                        torch.cuda.current_stream(self.device).cuda_stream))


GUIDE_ACTIVATIONS = {torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu", torch.nn.Mish: "mish"}


class GuideState:
    """A value model the library evaluates itself (dad_guide_grad, dad_guided_loop): an ``nn.Sequential`` of 2 to 4
    ``nn.Linear`` alternating with one of ``nn.Tanh`` / ``nn.ReLU`` / ``nn.Mish`` (the same throughout), ending in
    ``Linear(., 1)``, applied to the first ``in_dim`` channels of every horizon step and summed over the horizon
    (guides/policies.py:243-271).  Holds the zero-padded weight images, each in both orientations, and the
    ``dad_guide_args`` that point at them; :meth:`compile` builds one, :meth:`refresh` follows the module's parameters.
    """

    def __init__(self):
        raise TypeError("GuideState.compile(module, in_dim, device) builds a GuideState")

    @staticmethod
    def recognise(module, in_dim: int):
        """((Linear, ...), activation name) of a module of the supported form, or (None, why not)."""
        nn = torch.nn
        if not isinstance(module, nn.Sequential):
            return None, f"the value model is a {type(module).__name__}, not an nn.Sequential"
        mods = list(module)
        if len(mods) % 2 == 0 or not all(isinstance(m, nn.Linear) for m in mods[0::2]):
            return None, "the value model does not alternate nn.Linear with an activation, ending in nn.Linear"
        linears, acts = mods[0::2], mods[1::2]
        if not acts:
            return None, "the value model has no hidden layer"
        kinds = {type(a) for a in acts}
        if len(kinds) != 1 or next(iter(kinds)) not in GUIDE_ACTIVATIONS:
            return None, ("the activations are " + ", ".join(sorted(k.__name__ for k in kinds)) +
                          ": one of nn.Tanh, nn.ReLU, nn.Mish throughout is needed")
        if linears[0].in_features != int(in_dim):
            return None, f"the first layer reads {linears[0].in_features} features, the guide is given {int(in_dim)}"
        for a, b in zip(linears, linears[1:]):
            if b.in_features != a.out_features:
                return None, f"layer widths do not chain ({a.out_features} -> {b.in_features})"
        if linears[-1].out_features != 1:
            return None, f"the last layer has {linears[-1].out_features} outputs, not 1"
        for p in module.parameters():
            if p.dtype != torch.float32:
                return None, f"a parameter is {p.dtype}, not float32"
        return tuple(linears), GUIDE_ACTIVATIONS[next(iter(kinds))]

    @classmethod
    def compile(cls, module, in_dim: int, device=None, *, host: bool = False):
        """``(state, None)``, or ``(None, reason)`` for a module the library does not evaluate.  ``device``: where the
        engine runs; the parameters must live there.  ``host``: recognise and plan only, no device (CPU modules):
        enough for :meth:`plan`."""
        linears, act = cls.recognise(module, in_dim)
        if linears is None:
            return None, act
        widths = [int(l.out_features) for l in linears]
        plan = guide_plan(in_dim, widths, act, 1, 1)
        if plan["refused"] is not None:
            return None, f"the planner refuses the net: {plan['refused']} (in_dim {in_dim}, widths {widths}, {act})"
        dev = None
        if not host:
            dev = torch.device(device)
            if dev.type != "cuda":
                raise RuntimeError("the guide kernel needs a ROCm device; there is no CPU path")
            for p in module.parameters():
                if p.device != dev:
                    return None, f"a parameter lives on {p.device}, the engine on {dev}"
        self = cls.__new__(cls)
        self.module, self.linears, self.activation = module, linears, act
        self.in_dim, self.widths, self.padded = int(in_dim), widths, plan["padded"]
        self.device, self._dirty, self._key, self._scratch = dev, True, None, None
        a = DadGuideArgs()
        a.n_layers, a.in_dim = len(widths), int(in_dim)
        a.activation = _names("DAD_GD_ACTS").index(act)
        for i, w in enumerate(widths):
            a.widths[i] = w
        for i, w in enumerate(self.padded):
            a.padded[i] = w
        self.args = a
        self._images = None
        if not host:
            L, pad = len(widths), self.padded
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            self._images = [(z(pad[i], pad[i + 1]), z(pad[i + 1], pad[i]), z(pad[i + 1])) for i in range(L - 1)]
            self._images.append((z(pad[L - 1]), None, z(1)))
            for i, (wf, wb, b) in enumerate(self._images):
                a.w_fwd[i], a.w_bwd[i], a.bias[i] = wf.data_ptr(), _ptr(wb), b.data_ptr()
            self.refresh()
        return self, None

    def _param_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.module.parameters())

    def mark_changed(self) -> None:
        """Tell the state that parameter values changed without their versions (a ``.data`` update), as
        ``TemporalUnet.mark_weights_changed`` does for the denoiser."""
        self._dirty = True

    def refresh(self) -> None:
        """Rebuild the padded images, in place (captured loops keep their pointers and follow the values), when any
        parameter's (data_ptr, _version) changed or :meth:`mark_changed` was called."""
        if self._images is None:
            return
        key = self._param_key()
        if not self._dirty and key == self._key:
            return
        with torch.no_grad():
            L = len(self.linears)
            for i, (lin, (wf, wb, b)) in enumerate(zip(self.linears, self._images)):
                n, k = lin.weight.shape
                if i < L - 1:
                    wf[:k, :n].copy_(lin.weight.detach().t())
                    wb[:n, :k].copy_(lin.weight.detach())
                    b[:n].copy_(lin.bias.detach()) if lin.bias is not None else b.zero_()
                else:
                    wf[:k].copy_(lin.weight.detach()[0])
                    b.copy_(lin.bias.detach()) if lin.bias is not None else b.zero_()
        self._key, self._dirty = key, False

    def plan(self, batch: int, horizon: int, transition_dim: Optional[int] = None) -> dict:
        """What one guide launch is for ``batch`` trajectories of ``horizon`` steps (:func:`guide_plan`; no device)."""
        return guide_plan(self.in_dim, self.widths, self.activation, batch, horizon, transition_dim)

    def bind_scratch(self, scratch: Optional[torch.Tensor], x: torch.Tensor) -> None:
        """Point ``dad_guide_args.grad`` at ``scratch`` (as large as ``x``), or at a buffer of the state's own."""
        if scratch is None:
            if self._scratch is None or self._scratch.numel() < x.numel():
                self._scratch = torch.empty(x.numel(), dtype=torch.float32, device=self.device)
            scratch = self._scratch
        self.args.grad, self.args.grad_bytes = scratch.data_ptr(), scratch.numel() * 4

    def grad(self, x: torch.Tensor, value_rows: bool = False):
        """d/dx of sum over the horizon of the value model on ``x[..., :in_dim]``, (B, H, td) (dad_guide_grad: one
        launch, asynchronous); with ``value_rows`` also the per-row values (B, H)."""
        _require_device(x, "x")
        if x.dim() != 3 or x.shape[2] < self.in_dim:
            raise RuntimeError(f"x must be (B, H, td >= {self.in_dim}), got {tuple(x.shape)}")
        if x.device != self.device:
            raise RuntimeError(f"x is on {x.device}, the guide on {self.device}")
        self.refresh()
        g = torch.empty_like(x)
        v = torch.empty(x.shape[:2], dtype=torch.float32, device=x.device) if value_rows else None
        lib = load_library()
        with torch.cuda.device(self.device):
            _check(lib, lib.dad_guide_grad(C.byref(self.args), x.data_ptr(), g.data_ptr(), _ptr(v), int(x.shape[0]),
                                           int(x.shape[1]), int(x.shape[2]),
                                           torch.cuda.current_stream(self.device).cuda_stream))
        return (g, v) if value_rows else g
