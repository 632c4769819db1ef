"""Every forward kernel the planner can reach, run against float64.

tests/forward_census.py (a manual, host-only tool) walks a bounded space of architectures, batches, forced tiles, debug
options and the four call modes of HipEngine.forward_plan (dad_debug_forward_plan: the description the entry points
replay), and picks by greedy set cover the CASES below; NOT_REACHED lists the registered kernels nothing in that space
launches ("not reached in this space", not "dead": DESIGN.md, "Forward kernel census").

(a) test_matrix_reaches_every_forward_path (no device): every case's plan, under its own options, holds the kernel keys
    and path features the case exists for; the kernels the matrix launches and NOT_REACHED are disjoint and together are
    the whole domain of kernel_registered (335) and of the small-batch kernels (18 conv_cc + 20 conv_ccw); and the matrix
    covers every gn_pass_kernel<npt> the planner can produce, grid split-K on and off on every tile that supports it, a
    partly empty last N tile on every tile, final_gy > 1, final_cc_kernel, res_kind 1..4, and BIG / ride_in small-batch
    launches on 16- and 32-row tiles.  A retuned planner that moves a case off its path, or that makes a listed kernel
    reachable from the matrix, fails here.
(b) test_forward_case_vs_float64 (gpu): each case builds its net with synthetic weights (GroupNorm gamma / beta and the
    biases off their defaults), asserts its keys on the plan of the engine that runs, and compares with oracle.denoiser
    on cast_weights(w, float64): modes 0 / 1 / 2 the output at TOL_STEP (5e-6 absolute; mode 1 on distinct per-row
    timesteps), mode 3 d loss / d x_t and every parameter gradient at REL = 2e-5 max|g_f64| (scales of
    tests/util.py::grad_scales).  Both gates are those of tests/test_hip_train_batch.py; the fp32 oracle's own distance is
    printed beside the engine's.  A second call gives the same bits.

The census (13 932 architectures, 86 506 distinct plans) reaches 311 of the 335 conv-GEMM kernels, 12 of 18 conv_cc and 12 of
20 conv_ccw instantiations; the 103 cases launch all of them but the three conv-GEMM kernels of
the finding below, which the planner has stopped launching (308 since); NOT_REACHED holds those three and the other 38.

Measured on an MI355X (`-s` prints every case; 62 s for the file): outputs of modes 0 / 1 / 2 are 2.0e-7 .. 2.3e-6 from the
float64 forward (worst: k7_d128_m1421_H256_td6_fp32_B1_mode0_t102, the windowed 7-tap tile-2 case), the fp32 oracle 3.4e-7 ..
4.2e-6; mode 3 gradients 1.3e-6 .. 1.7e-5 x max|g| (worst: k7_d32_m1421_H8_td6_fp32_B1_mode3_t2, four levels at horizon 8: one
real position at the deepest level), the fp32 oracle 2.3e-6 .. 1.7e-5.

A FINDING of these cases: conv_gemm_f32<32, 64, 2, 16, k, 1, RAGGED = false, ..., RES = true> -- ("gemm", 5, k, 1, 8): the 1x1
residual conv riding in its carrier on tile 5 with whole K chunks -- computes wrong values.  Only dad_debug_set_tile(5 / 105)
reached it (choose_tile never picks tile 5), on a block with a residual conv behind 16-channel-aligned inputs; with it
    k5_d256_m1248_H32_td6_fp32_B1_mode1_t105   was 2.25e-01 .. 2.52e-01 from float64 (the fp32 oracle 1.31e-06)
    k7_d64_m18_H16_td6_fp32_B1_mode0_t105          2.31e-01                              (2.47e-06)
    k3_d64_m18_H8_td6_fp32_B1_mode0_t105           2.68e-01                              (1.34e-06)
and single-level probes (transition_dim 16 / 32, dim 32 / 64, one or two K chunks, batch 1 and 8, 3 and 5 taps) 0.14 .. 0.24,
0.07 even with the weights of both convs zero, where the same nets on tile 6 (32 x 64 without the second split-K wave) are
3e-7 .. 5e-7; the RAGGED twin ("gemm", 5, k, 1, 12), tile 5 without the ride and the ride on every other tile pass.  Its cause
is not found, so the planner no longer launches the form (fused_at of host_plan.hpp: on tile 5 with whole chunks the 1x1 conv
runs on its own); the three kernels stay registered and are listed in NOT_REACHED, and the three cases pass at the gate (8.4e-7 .. 1.4e-6).

Each of three deliberate one-line errors (scratch builds, none committed), each in a form the earlier GPU suite does not reach,
made exactly the cases fail that launch the form:
    conv_gemm.hpp, WIN: the window's first input position + 1 where TAPS == 7 and BM == 128
        -> k7_d128_m1421_H256_td6_fp32_B1_mode0_t102
    conv_gemm.hpp, PADDED: weight tap slot 3 staged for slot 2 where TAPS == 7, BM == 64, BN == 128 (tile 9)
        -> k7_d256_m148_H24_td6_fp32_B1_mode0_t9
    conv_gemm.hpp: weight tap slot 2 staged for slot 1 in the plain 3-tap stride-1 form of tile 7 (tiles 5 .. 7 run only when
    forced, and the earlier suite forces them on 5-tap nets alone)
        -> k3_d32_m12_H8_td6_fp32_B1_mode0_t107, k3_d64_m1_H8_td6_fp32_B1_mode0_t7, k3_d64_m1_H8_td6_fp32_B1_mode0_t7_fuse_residual0,
           k3_d64_m11_H8_td6_fp32_B1_mode3_t7
With the first two in the library the earlier GPU suite noticed neither.  A fourth error, cc_build_input_gn's second round
trip skipped (BIG: an input in 9..16 slabs), fails k5_d128_m148_H64_td64_fp32_B1_mode0_t-1 and
k5_d256_m1248_H32_td6_fp32_B1_mode0_t-1 here, but the earlier suite reaches BIG too (PointMaze and Door at small batches:
20 of its tests failed), so it does not count as a gap closed.
"""
import functools

import numpy as np
import pytest
import torch

from tests import forward_census as census
from tests.test_hip_parity import TOL_STEP, dev  # noqa: F401  (dev: fixture)
from tests.util import as_torch, grad_scales, max_abs

REL = 2e-5
T = census.T
KERNEL_FAMILIES = ("gemm", "cc", "ccw")

# (id, td, dim, mults, horizon (real: the engine pads 24 / 100 / 200 / 384, and the widths of dim 48 / 96), kernel_size,
#  precision, batch, mode, tile, options off their defaults, keys it exists for)
CASES = [
    ('k5_d32_m1421_H512_td6_f16x3_B1_mode0_t1', 6, 32, (1, 4, 2, 1), 512, 5, 'f16x3', 1, 0, 1, {},
     [('gemm', 0, 1, 1, 5), ('gemm', 0, 1, 1, 48), ('gemm', 0, 1, 1, 52), ('gemm', 0, 2, 1, 48), ('gemm', 0, 3, 2, 48), ('gemm', 0, 5, 1, 1), ('gemm', 0, 5, 1, 5), ('gemm', 0, 5, 1, 48), ('gemm', 0, 5, 1, 52), ('gemm', 1, 1, 1, 52), ('gemm', 1, 2, 1, 1), ('gemm', 1, 3, 2, 1), ('gemm', 1, 5, 1, 1), ('gemm', 1, 5, 1, 48), ('gemm', 8, 1, 1, 1), ('gemm', 8, 2, 1, 1), ('gemm', 8, 3, 2, 1), ('gemm', 8, 5, 1, 1), ('gn_npt', 1), ('gn_npt', 2), ('gn_npt', 4), ('split', 0, 0), ('split', 0, 1), ('split', 1, 0), ('split', 1, 1), ('split', 8, 1)]),
    ('k5_d128_m148_H64_td64_fp32_B1_mode0_t-1', 64, 128, (1, 4, 8), 64, 5, 'fp32', 1, 0, -1, {},
     [('big', 32), ('cc', 2, 1, 0, 0, 16, 0), ('cc', 2, 1, 0, 0, 32, 0), ('cc', 3, 2, 0, 0, 32, 0), ('cc', 5, 1, 0, 0, 16, 0), ('cc', 5, 1, 0, 0, 32, 0), ('cc', 5, 1, 0, 0, 32, 1), ('cc', 5, 1, 0, 1, 32, 0), ('cc', 5, 1, 1, 0, 16, 0), ('cc', 5, 1, 1, 0, 32, 0), ('cc', 5, 1, 1, 0, 32, 1), ('ccw', 3, 2, 0, 0, 16), ('ccw', 5, 1, 0, 0, 16), ('ccw', 5, 1, 0, 0, 32), ('ccw', 5, 1, 0, 1, 16), ('ccw', 5, 1, 0, 1, 32), ('ccw', 5, 1, 1, 0, 16), ('final_cc',), ('final_gy>1', 'final_cc_kernel'), ('res_kind', 0), ('res_kind', 2), ('res_kind', 3), ('ride_in', 16), ('ride_in', 32)]),
    ('k3_d32_m1224_H256_td6_fp32_B1_mode0_t2', 6, 32, (1, 2, 2, 4), 256, 3, 'fp32', 1, 0, 2, {},
     [('gemm', 0, 1, 1, 0), ('gemm', 0, 1, 1, 4), ('gemm', 0, 2, 1, 0), ('gemm', 0, 3, 1, 0), ('gemm', 0, 3, 1, 48), ('gemm', 0, 3, 1, 52), ('gemm', 0, 3, 2, 0), ('gemm', 2, 1, 1, 0), ('gemm', 2, 3, 1, 0), ('gemm', 8, 1, 1, 0), ('gemm', 8, 2, 1, 0), ('gemm', 8, 3, 1, 0), ('gemm', 8, 3, 1, 8), ('gemm', 8, 3, 2, 0), ('part_tile', 0), ('part_tile', 2), ('split', 2, 0), ('split', 2, 1), ('split', 8, 0)]),
    ('k3_d128_m1421_H384_td6_fp32_B1_mode0_t102', 6, 128, (1, 4, 2, 1), 384, 3, 'fp32', 1, 0, 102, {},
     [('gemm', 2, 1, 1, 16), ('gemm', 2, 1, 1, 48), ('gemm', 2, 1, 1, 52), ('gemm', 2, 2, 1, 16), ('gemm', 2, 2, 1, 48), ('gemm', 2, 3, 1, 16), ('gemm', 2, 3, 1, 48), ('gemm', 2, 3, 1, 52), ('gemm', 2, 3, 2, 16), ('gemm', 2, 3, 2, 48), ('gemm', 8, 1, 1, 16), ('gemm', 8, 2, 1, 16), ('gemm', 8, 3, 1, 16), ('gemm', 8, 3, 2, 16), ('gemm', 9, 3, 1, 16), ('gn_npt', 8), ('gn_npt', 16), ('split', 9, 0)]),
    ('k5_d32_m124_H100_td6_fp32_B1_mode0_t4', 6, 32, (1, 2, 4), 100, 5, 'fp32', 1, 0, 4, {},
     [('gemm', 0, 1, 1, 20), ('gemm', 0, 2, 1, 16), ('gemm', 0, 3, 2, 16), ('gemm', 0, 5, 1, 16), ('gemm', 4, 1, 1, 16), ('gemm', 4, 1, 1, 20), ('gemm', 4, 2, 1, 16), ('gemm', 4, 3, 2, 16), ('gemm', 4, 5, 1, 16), ('gemm', 8, 1, 1, 20), ('gemm', 8, 5, 1, 16), ('gemm', 8, 5, 1, 20), ('part_tile', 4), ('split', 4, 0), ('split', 4, 1)]),
    ('k5_d256_m1248_H32_td6_fp32_B1_mode1_t105', 6, 256, (1, 2, 4, 8), 32, 5, 'fp32', 1, 1, 105, {},
     [('gemm', 1, 5, 1, 0), ('gemm', 1, 5, 1, 8), ('gemm', 2, 5, 1, 0), ('gemm', 2, 5, 1, 8), ('gemm', 3, 5, 1, 2), ('gemm', 5, 1, 1, 0), ('gemm', 5, 2, 1, 0), ('gemm', 5, 3, 2, 0), ('gemm', 5, 5, 1, 0), ('gemm', 5, 5, 1, 12), ('part_tile', 1), ('part_tile', 3), ('part_tile', 5), ('split', 3, 0), ('split', 5, 0)]),
    ('k7_d32_m1224_H128_td6_f16x3_B1_mode0_t6', 6, 32, (1, 2, 2, 4), 128, 7, 'f16x3', 1, 0, 6, {},
     [('gemm', 6, 1, 1, 1), ('gemm', 6, 1, 1, 5), ('gemm', 6, 2, 1, 0), ('gemm', 6, 2, 1, 1), ('gemm', 6, 3, 2, 0), ('gemm', 6, 3, 2, 1), ('gemm', 6, 7, 1, 0), ('gemm', 8, 1, 1, 5), ('gemm', 8, 7, 1, 0), ('gemm', 8, 7, 1, 4), ('part_tile', 6), ('split', 6, 0), ('split', 6, 1)]),
    ('k5_d32_m1224_H128_td6_fp32_B1_mode0_t7_fuse_residual0', 6, 32, (1, 2, 2, 4), 128, 5, 'fp32', 1, 0, 7, {'fuse_residual': 0},
     [('gemm', 0, 5, 1, 0), ('gemm', 7, 1, 1, 0), ('gemm', 7, 1, 1, 4), ('gemm', 7, 2, 1, 0), ('gemm', 7, 3, 2, 0), ('gemm', 7, 5, 1, 0), ('gemm', 8, 1, 1, 4), ('gemm', 8, 5, 1, 0), ('gemm', 8, 5, 1, 4), ('part_tile', 7), ('split', 7, 0), ('split', 7, 1)]),
    ('k5_d256_m1248_H8_td6_fp32_B1_mode0_t9', 6, 256, (1, 2, 4, 8), 8, 5, 'fp32', 1, 0, 9, {},
     [('gemm', 2, 5, 1, 16), ('gemm', 3, 5, 1, 18), ('gemm', 9, 1, 1, 16), ('gemm', 9, 1, 1, 20), ('gemm', 9, 2, 1, 16), ('gemm', 9, 3, 2, 16), ('gemm', 9, 5, 1, 16), ('gemm', 9, 5, 1, 20), ('part_tile', 9), ('split', 3, 1), ('split', 9, 1)]),
    ('k7_d64_m148_H16_td6_fp32_B1_mode0_t101', 6, 64, (1, 4, 8), 16, 7, 'fp32', 1, 0, 101, {},
     [('gemm', 0, 7, 1, 0), ('gemm', 0, 7, 1, 8), ('gemm', 1, 1, 1, 0), ('gemm', 1, 1, 1, 4), ('gemm', 1, 2, 1, 0), ('gemm', 1, 3, 2, 0), ('gemm', 1, 7, 1, 0), ('gemm', 1, 7, 1, 4), ('gemm', 4, 7, 1, 0), ('gemm', 4, 7, 1, 8)]),
    ('k7_d64_m1224_H384_td6_fp32_B1_mode0_t101', 6, 64, (1, 2, 2, 4), 384, 7, 'fp32', 1, 0, 101, {},
     [('gemm', 1, 1, 1, 16), ('gemm', 1, 1, 1, 48), ('gemm', 1, 2, 1, 16), ('gemm', 1, 2, 1, 48), ('gemm', 1, 3, 2, 16), ('gemm', 1, 3, 2, 48), ('gemm', 1, 7, 1, 16), ('gemm', 1, 7, 1, 48), ('gemm', 1, 7, 1, 52), ('gemm', 8, 7, 1, 16)]),
    ('k7_d32_m1248_H256_td6_f16x3_B1_mode0_t2', 6, 32, (1, 2, 4, 8), 256, 7, 'f16x3', 1, 0, 2, {},
     [('gemm', 0, 1, 1, 1), ('gemm', 0, 2, 1, 1), ('gemm', 0, 3, 2, 1), ('gemm', 0, 7, 1, 48), ('gemm', 0, 7, 1, 52), ('gemm', 2, 1, 1, 1), ('gemm', 2, 2, 1, 1), ('gemm', 2, 3, 2, 1), ('gemm', 2, 7, 1, 0)]),
    ('k3_d256_m1248_H32_td6_f16x3_B1_mode0_t5', 6, 256, (1, 2, 4, 8), 32, 3, 'f16x3', 1, 0, 5, {},
     [('gemm', 1, 3, 1, 0), ('gemm', 3, 3, 1, 3), ('gemm', 5, 1, 1, 1), ('gemm', 5, 1, 1, 5), ('gemm', 5, 2, 1, 1), ('gemm', 5, 3, 1, 0), ('gemm', 5, 3, 1, 4), ('gemm', 5, 3, 2, 1), ('split', 5, 1)]),
    ('k3_d256_m148_H16_td6_fp32_B1_mode0_t104', 6, 256, (1, 4, 8), 16, 3, 'fp32', 1, 0, 104, {},
     [('gemm', 2, 3, 1, 8), ('gemm', 3, 3, 1, 2), ('gemm', 4, 1, 1, 0), ('gemm', 4, 2, 1, 0), ('gemm', 4, 3, 1, 0), ('gemm', 4, 3, 1, 8), ('gemm', 4, 3, 1, 12), ('gemm', 4, 3, 2, 0)]),
    ('k5_d256_m148_H16_td6_f16x3_B1_mode0_t4', 6, 256, (1, 4, 8), 16, 5, 'f16x3', 1, 0, 4, {},
     [('gemm', 2, 5, 1, 1), ('gemm', 3, 5, 1, 3), ('gemm', 4, 1, 1, 1), ('gemm', 4, 1, 1, 5), ('gemm', 4, 2, 1, 1), ('gemm', 4, 3, 2, 1), ('gemm', 4, 5, 1, 1), ('gemm', 4, 5, 1, 5)]),
    ('k5_d32_m1224_H128_td64_fp32_B1_mode0_t109', 64, 32, (1, 2, 2, 4), 128, 5, 'fp32', 1, 0, 109, {},
     [('final_gy>1', 'final_posterior_kernel'), ('gemm', 0, 5, 1, 8), ('gemm', 8, 5, 1, 8), ('gemm', 9, 2, 1, 0), ('gemm', 9, 3, 2, 0), ('gemm', 9, 5, 1, 0), ('gemm', 9, 5, 1, 8)]),
    ('k3_d32_m1421_H384_td6_fp32_B1_mode3_t1', 6, 32, (1, 4, 2, 1), 384, 3, 'fp32', 1, 3, 1, {},
     [('gemm', 0, 3, 1, 16), ('gemm', 0, 5, 2, 48), ('gemm', 1, 1, 1, 20), ('gemm', 1, 3, 1, 16), ('gemm', 1, 3, 1, 48), ('gemm', 1, 5, 2, 16), ('gemm', 8, 5, 2, 16)]),
    ('k7_d256_m18_H8_td6_f16x3_B1_mode0_t7', 6, 256, (1, 8), 8, 7, 'f16x3', 1, 0, 7, {},
     [('gemm', 3, 7, 1, 3), ('gemm', 7, 1, 1, 1), ('gemm', 7, 1, 1, 5), ('gemm', 7, 2, 1, 1), ('gemm', 7, 3, 2, 1), ('gemm', 7, 7, 1, 0), ('gemm', 7, 7, 1, 4)]),
    ('k3_d64_m11_H8_td6_f16x3_B1_mode0_t9', 6, 64, (1, 1), 8, 3, 'f16x3', 1, 0, 9, {},
     [('gemm', 9, 1, 1, 1), ('gemm', 9, 1, 1, 5), ('gemm', 9, 2, 1, 1), ('gemm', 9, 3, 1, 0), ('gemm', 9, 3, 1, 4), ('gemm', 9, 3, 2, 1)]),
    ('k7_d32_m1421_H8_td6_fp32_B1_mode3_t2', 6, 32, (1, 4, 2, 1), 8, 7, 'fp32', 1, 3, 2, {},
     [('gemm', 0, 1, 1, 16), ('gemm', 0, 5, 2, 16), ('gemm', 0, 7, 1, 16), ('gemm', 2, 1, 1, 20), ('gemm', 2, 5, 2, 16), ('gemm', 2, 7, 1, 16)]),
    ('k7_d128_m1421_H256_td6_fp32_B1_mode0_t102', 6, 128, (1, 4, 2, 1), 256, 7, 'fp32', 1, 0, 102, {},
     [('gemm', 2, 2, 1, 0), ('gemm', 2, 3, 2, 0), ('gemm', 2, 7, 1, 48), ('gemm', 2, 7, 1, 52), ('gemm', 8, 7, 1, 8), ('gemm', 9, 7, 1, 0), ('gemm', 9, 7, 1, 8)]),
    ('k5_d256_m1248_H32_td6_fp32_B1_mode0_t-1', 6, 256, (1, 2, 4, 8), 32, 5, 'fp32', 1, 0, -1, {},
     [('big', 16), ('cc', 3, 2, 0, 0, 16, 0), ('cc', 5, 1, 0, 1, 16, 0), ('ccw', 1, 1, 0, 0, 16), ('ccw', 2, 1, 0, 0, 16), ('res_kind', 4)]),
    ('k3_d32_m1224_H256_td6_fp32_B1_mode3_t6', 6, 32, (1, 2, 2, 4), 256, 3, 'fp32', 1, 3, 6, {},
     [('gemm', 6, 1, 1, 0), ('gemm', 6, 1, 1, 4), ('gemm', 6, 3, 1, 0), ('gemm', 6, 5, 2, 0), ('gemm', 8, 5, 2, 0)]),
    ('k3_d32_m12_H8_td6_fp32_B1_mode0_t107', 6, 32, (1, 2), 8, 3, 'fp32', 1, 0, 107, {},
     [('gemm', 0, 3, 1, 8), ('gemm', 0, 3, 1, 12), ('gemm', 7, 3, 1, 0), ('gemm', 7, 3, 1, 8)]),
    ('k5_d32_m124_H16_td6_fp32_B1_mode3_t4', 6, 32, (1, 2, 4), 16, 5, 'fp32', 1, 3, 4, {},
     [('gemm', 0, 5, 2, 0), ('gemm', 4, 1, 1, 4), ('gemm', 4, 5, 1, 0), ('gemm', 4, 5, 2, 0)]),
    ('k7_d64_m18_H16_td6_fp32_B1_mode0_t105', 6, 64, (1, 8), 16, 7, 'fp32', 1, 0, 105, {},
     [('gemm', 5, 1, 1, 4), ('gemm', 5, 7, 1, 0), ('gemm', 5, 7, 1, 12)]),
    ('k7_d256_m18_H8_td6_fp32_B1_mode0_t9_fuse_residual0', 6, 256, (1, 8), 8, 7, 'fp32', 1, 0, 9, {'fuse_residual': 0},
     [('gemm', 3, 7, 1, 2), ('gemm', 9, 1, 1, 0), ('gemm', 9, 1, 1, 4), ('gemm', 9, 7, 1, 4)]),
    ('k5_d32_m11_H8_td6_fp32_B1_mode1_t106', 6, 32, (1, 1), 8, 5, 'fp32', 1, 1, 106, {},
     [('gemm', 6, 5, 1, 0), ('gemm', 6, 5, 1, 8), ('gemm', 6, 5, 1, 12)]),
    ('k3_d64_m12_H8_td6_f16x3_B1_mode0_t1', 6, 64, (1, 2), 8, 3, 'f16x3', 1, 0, 1, {},
     [('gemm', 1, 1, 1, 1), ('gemm', 1, 1, 1, 5), ('gemm', 1, 3, 1, 4)]),
    ('k3_d64_m18_H8_td6_fp32_B1_mode0_t105', 6, 64, (1, 8), 8, 3, 'fp32', 1, 0, 105, {},
     [('gemm', 1, 3, 1, 8), ('gemm', 5, 3, 1, 12)]),
    ('k7_d64_m1248_H8_td6_fp32_B1_mode0_t8', 6, 64, (1, 2, 4, 8), 8, 7, 'fp32', 1, 0, 8, {},
     [('gemm', 4, 7, 1, 16), ('gemm', 8, 7, 1, 20), ('part_tile', 8)]),
    ('k3_d256_m1248_H8_td6_fp32_B1_mode0_t4', 6, 256, (1, 2, 4, 8), 8, 3, 'fp32', 1, 0, 4, {},
     [('gemm', 3, 3, 1, 18), ('gemm', 4, 3, 1, 16), ('gemm', 4, 3, 1, 20)]),
    ('k5_d128_m1421_H256_td6_f16x3_B1_mode0_t2', 6, 128, (1, 4, 2, 1), 256, 5, 'f16x3', 1, 0, 2, {},
     [('gemm', 2, 5, 1, 48), ('gemm', 2, 5, 1, 52), ('gemm', 9, 5, 1, 1)]),
    ('k5_d256_m148_H16_td6_fp32_B5_mode0_t-1_ccw_min_blocks4096', 6, 256, (1, 4, 8), 16, 5, 'fp32', 5, 0, -1, {'ccw_min_blocks': 4096},
     [('ccw', 1, 1, 0, 0, 32), ('ccw', 2, 1, 0, 0, 32), ('ccw', 3, 2, 0, 0, 32), ('ccw', 5, 1, 1, 0, 32)]),
    ('k7_d256_m148_H24_td6_fp32_B1_mode0_t9', 6, 256, (1, 4, 8), 24, 7, 'fp32', 1, 0, 9, {},
     [('gemm', 3, 7, 1, 18), ('gemm', 9, 7, 1, 16), ('gemm', 9, 7, 1, 20)]),
    ('k3_d32_m11_H8_td6_fp32_B1_mode0_t106', 6, 32, (1, 1), 8, 3, 'fp32', 1, 0, 106, {},
     [('gemm', 6, 3, 1, 8), ('gemm', 6, 3, 1, 12)]),
    ('k5_d32_m1_H8_td6_f16x3_B1_mode0_t5', 6, 32, (1,), 8, 5, 'f16x3', 1, 0, 5, {},
     [('gemm', 5, 5, 1, 1), ('gemm', 5, 5, 1, 5)]),
    ('k5_d32_m1_H8_td6_f16x3_B1_mode0_t6', 6, 32, (1,), 8, 5, 'f16x3', 1, 0, 6, {},
     [('gemm', 6, 5, 1, 1), ('gemm', 6, 5, 1, 5)]),
    ('k7_d32_m11_H8_td6_fp32_B1_mode0_t106', 6, 32, (1, 1), 8, 7, 'fp32', 1, 0, 106, {},
     [('gemm', 6, 7, 1, 8), ('gemm', 6, 7, 1, 12)]),
    ('k5_d32_m112_H8_td6_fp32_B1_mode0_t1', 6, 32, (1, 1, 2), 8, 5, 'fp32', 1, 0, 1, {},
     [('gemm', 0, 5, 1, 20), ('gemm', 1, 5, 1, 16)]),
    ('k5_d32_m12_H8_td6_fp32_B1_mode1_t104', 6, 32, (1, 2), 8, 5, 'fp32', 1, 1, 104, {},
     [('gemm', 0, 5, 1, 12), ('gemm', 4, 5, 1, 8)]),
    ('k3_d64_m11_H8_td6_fp32_B1_mode0_t109', 6, 64, (1, 1), 8, 3, 'fp32', 1, 0, 109, {},
     [('gemm', 9, 3, 1, 8), ('gemm', 9, 3, 1, 12)]),
    ('k5_d64_m1_H8_td6_f16x3_B1_mode0_t7', 6, 64, (1,), 8, 5, 'f16x3', 1, 0, 7, {},
     [('gemm', 7, 5, 1, 1), ('gemm', 7, 5, 1, 5)]),
    ('k7_d32_m12_H8_td6_fp32_B1_mode0_t107', 6, 32, (1, 2), 8, 7, 'fp32', 1, 0, 107, {},
     [('gemm', 0, 7, 1, 12), ('gemm', 7, 7, 1, 8)]),
    ('k5_d64_m11_H8_td6_fp32_B1_mode1_t107', 6, 64, (1, 1), 8, 5, 'fp32', 1, 1, 107, {},
     [('gemm', 7, 5, 1, 8), ('gemm', 7, 5, 1, 12)]),
    ('k3_d32_m14_H8_td6_fp32_B1_mode0_t2_fuse_residual0', 6, 32, (1, 4), 8, 3, 'fp32', 1, 0, 2, {'fuse_residual': 0},
     [('gemm', 0, 3, 1, 4), ('gemm', 2, 1, 1, 4)]),
    ('k3_d128_m1_H8_td6_f16x3_B1_mode0_t2', 6, 128, (1,), 8, 3, 'f16x3', 1, 0, 2, {},
     [('gemm', 2, 1, 1, 5), ('gemm', 2, 3, 1, 4)]),
    ('k3_d64_m1224_H512_td6_fp32_B1_mode3_t101', 6, 64, (1, 2, 2, 4), 512, 3, 'fp32', 1, 3, 101, {},
     [('gemm', 1, 5, 2, 0), ('gemm', 1, 5, 2, 48)]),
    ('k3_d128_m1224_H512_td6_fp32_B1_mode3_t102', 6, 128, (1, 2, 2, 4), 512, 3, 'fp32', 1, 3, 102, {},
     [('gemm', 2, 5, 2, 0), ('gemm', 2, 5, 2, 48)]),
    ('k3_d128_m18_H384_td6_fp32_B1_mode0_t1', 6, 128, (1, 8), 384, 3, 'fp32', 1, 0, 1, {},
     [('gemm', 1, 3, 1, 52), ('gn_npt', 32)]),
    ('k3_d32_m1_H8_td6_fp32_B1_mode0_t6_fuse_residual0', 6, 32, (1,), 8, 3, 'fp32', 1, 0, 6, {'fuse_residual': 0},
     [('gemm', 6, 3, 1, 4)]),
    ('k3_d32_m1_H8_td6_fp32_B1_mode0_t8', 6, 32, (1,), 8, 3, 'fp32', 1, 0, 8, {},
     [('gemm', 8, 3, 1, 12)]),
    ('k3_d32_m1_H8_td6_fp32_B1_mode0_t8_fuse_residual0', 6, 32, (1,), 8, 3, 'fp32', 1, 0, 8, {'fuse_residual': 0},
     [('gemm', 8, 3, 1, 4)]),
    ('k5_d32_m1_H8_td6_fp32_B1_mode1_t-1_fuse_residual0', 6, 32, (1,), 8, 5, 'fp32', 1, 1, -1, {'fuse_residual': 0},
     [('gemm', 0, 5, 1, 4)]),
    ('k5_d32_m1_H8_td6_fp32_B1_mode1_t5_fuse_residual0', 6, 32, (1,), 8, 5, 'fp32', 1, 1, 5, {'fuse_residual': 0},
     [('gemm', 5, 5, 1, 4)]),
    ('k5_d32_m1_H8_td6_fp32_B1_mode1_t6_fuse_residual0', 6, 32, (1,), 8, 5, 'fp32', 1, 1, 6, {'fuse_residual': 0},
     [('gemm', 6, 5, 1, 4)]),
    ('k5_d32_m1_H8_td6_fp32_B1_mode1_t8', 6, 32, (1,), 8, 5, 'fp32', 1, 1, 8, {},
     [('gemm', 8, 5, 1, 12)]),
    ('k5_d32_m1_H8_td6_f16x3_B1_mode0_t8', 6, 32, (1,), 8, 5, 'f16x3', 1, 0, 8, {},
     [('gemm', 8, 5, 1, 5)]),
    ('k5_d32_m1_H8_td32_fp32_B1_mode0_t-1', 32, 32, (1,), 8, 5, 'fp32', 1, 0, -1, {},
     [('res_kind', 1)]),
    ('k7_d32_m1_H8_td6_fp32_B1_mode0_t-1_fuse_residual0', 6, 32, (1,), 8, 7, 'fp32', 1, 0, -1, {'fuse_residual': 0},
     [('gemm', 0, 7, 1, 4)]),
    ('k7_d32_m1_H8_td6_fp32_B1_mode0_t5_fuse_residual0', 6, 32, (1,), 8, 7, 'fp32', 1, 0, 5, {'fuse_residual': 0},
     [('gemm', 5, 7, 1, 4)]),
    ('k7_d32_m1_H8_td6_fp32_B1_mode0_t6_fuse_residual0', 6, 32, (1,), 8, 7, 'fp32', 1, 0, 6, {'fuse_residual': 0},
     [('gemm', 6, 7, 1, 4)]),
    ('k7_d32_m1_H8_td6_fp32_B1_mode0_t8', 6, 32, (1,), 8, 7, 'fp32', 1, 0, 8, {},
     [('gemm', 8, 7, 1, 12)]),
    ('k3_d32_m112_H8_td6_fp32_B1_mode0_t8', 6, 32, (1, 1, 2), 8, 3, 'fp32', 1, 0, 8, {},
     [('gemm', 8, 3, 1, 20)]),
    ('k3_d32_m112_H8_td6_fp32_B1_mode0_t-1', 6, 32, (1, 1, 2), 8, 3, 'fp32', 1, 0, -1, {},
     [('gemm', 0, 3, 1, 20)]),
    ('k3_d64_m1_H8_td6_fp32_B1_mode0_t1', 6, 64, (1,), 8, 3, 'fp32', 1, 0, 1, {},
     [('gemm', 1, 3, 1, 12)]),
    ('k3_d64_m1_H8_td6_fp32_B1_mode0_t4_fuse_residual0', 6, 64, (1,), 8, 3, 'fp32', 1, 0, 4, {'fuse_residual': 0},
     [('gemm', 4, 3, 1, 4)]),
    ('k3_d64_m1_H8_td6_fp32_B1_mode0_t7', 6, 64, (1,), 8, 3, 'fp32', 1, 0, 7, {},
     [('gemm', 7, 3, 1, 12)]),
    ('k3_d64_m1_H8_td6_fp32_B1_mode0_t7_fuse_residual0', 6, 64, (1,), 8, 3, 'fp32', 1, 0, 7, {'fuse_residual': 0},
     [('gemm', 7, 3, 1, 4)]),
    ('k3_d48_m1_H8_td6_fp32_B1_mode0_t1', 6, 48, (1,), 8, 3, 'fp32', 1, 0, 1, {},
     [('gemm', 1, 3, 1, 20)]),
    ('k3_d48_m1_H8_td6_fp32_B1_mode0_t9', 6, 48, (1,), 8, 3, 'fp32', 1, 0, 9, {},
     [('gemm', 9, 3, 1, 20)]),
    ('k3_d32_m11_H8_td6_fp32_B1_mode3_t5', 6, 32, (1, 1), 8, 3, 'fp32', 1, 3, 5, {},
     [('gemm', 5, 5, 2, 0)]),
    ('k7_d32_m112_H8_td6_fp32_B1_mode0_t-1', 6, 32, (1, 1, 2), 8, 7, 'fp32', 1, 0, -1, {},
     [('gemm', 0, 7, 1, 20)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t1', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 1, {},
     [('gemm', 1, 5, 1, 12)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t1_fuse_residual0', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 1, {'fuse_residual': 0},
     [('gemm', 1, 5, 1, 4)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t4', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 4, {},
     [('gemm', 4, 5, 1, 12)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t4_fuse_residual0', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 4, {'fuse_residual': 0},
     [('gemm', 4, 5, 1, 4)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t7_fuse_residual0', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 7, {'fuse_residual': 0},
     [('gemm', 7, 5, 1, 4)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t9', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 9, {},
     [('gemm', 9, 5, 1, 12)]),
    ('k5_d64_m1_H8_td6_fp32_B1_mode1_t9_fuse_residual0', 6, 64, (1,), 8, 5, 'fp32', 1, 1, 9, {'fuse_residual': 0},
     [('gemm', 9, 5, 1, 4)]),
    ('k5_d64_m1_H8_td6_f16x3_B1_mode0_t1', 6, 64, (1,), 8, 5, 'f16x3', 1, 0, 1, {},
     [('gemm', 1, 5, 1, 5)]),
    ('k5_d64_m1_H8_td6_f16x3_B1_mode0_t9', 6, 64, (1,), 8, 5, 'f16x3', 1, 0, 9, {},
     [('gemm', 9, 5, 1, 5)]),
    ('k5_d48_m1_H8_td6_fp32_B1_mode0_t1', 6, 48, (1,), 8, 5, 'fp32', 1, 0, 1, {},
     [('gemm', 1, 5, 1, 20)]),
    ('k5_d48_m1_H8_td6_fp32_B1_mode0_t4', 6, 48, (1,), 8, 5, 'fp32', 1, 0, 4, {},
     [('gemm', 4, 5, 1, 20)]),
    ('k7_d64_m1_H8_td6_fp32_B1_mode0_t4', 6, 64, (1,), 8, 7, 'fp32', 1, 0, 4, {},
     [('gemm', 4, 7, 1, 12)]),
    ('k7_d64_m1_H8_td6_fp32_B1_mode0_t4_fuse_residual0', 6, 64, (1,), 8, 7, 'fp32', 1, 0, 4, {'fuse_residual': 0},
     [('gemm', 4, 7, 1, 4)]),
    ('k7_d64_m1_H8_td6_fp32_B1_mode0_t7', 6, 64, (1,), 8, 7, 'fp32', 1, 0, 7, {},
     [('gemm', 7, 7, 1, 12)]),
    ('k7_d64_m1_H8_td6_fp32_B1_mode0_t9', 6, 64, (1,), 8, 7, 'fp32', 1, 0, 9, {},
     [('gemm', 9, 7, 1, 12)]),
    ('k7_d48_m1_H8_td6_fp32_B1_mode0_t1', 6, 48, (1,), 8, 7, 'fp32', 1, 0, 1, {},
     [('gemm', 1, 7, 1, 20)]),
    ('k7_d48_m1_H8_td6_fp32_B1_mode0_t4', 6, 48, (1,), 8, 7, 'fp32', 1, 0, 4, {},
     [('gemm', 4, 7, 1, 20)]),
    ('k3_d128_m1_H8_td6_fp32_B1_mode0_t2', 6, 128, (1,), 8, 3, 'fp32', 1, 0, 2, {},
     [('gemm', 2, 3, 1, 12)]),
    ('k3_d96_m1_H8_td6_fp32_B1_mode0_t2', 6, 96, (1,), 8, 3, 'fp32', 1, 0, 2, {},
     [('gemm', 2, 3, 1, 20)]),
    ('k3_d64_m11_H8_td6_fp32_B1_mode3_t7', 6, 64, (1, 1), 8, 3, 'fp32', 1, 3, 7, {},
     [('gemm', 7, 5, 2, 0)]),
    ('k3_d64_m11_H8_td6_fp32_B1_mode3_t9', 6, 64, (1, 1), 8, 3, 'fp32', 1, 3, 9, {},
     [('gemm', 9, 5, 2, 0)]),
    ('k3_d48_m11_H8_td6_fp32_B1_mode3_t4', 6, 48, (1, 1), 8, 3, 'fp32', 1, 3, 4, {},
     [('gemm', 4, 5, 2, 16)]),
    ('k3_d48_m11_H8_td6_fp32_B1_mode3_t9', 6, 48, (1, 1), 8, 3, 'fp32', 1, 3, 9, {},
     [('gemm', 9, 5, 2, 16)]),
    ('k5_d128_m1_H8_td6_fp32_B1_mode1_t2', 6, 128, (1,), 8, 5, 'fp32', 1, 1, 2, {},
     [('gemm', 2, 5, 1, 12)]),
    ('k5_d128_m1_H8_td6_fp32_B1_mode1_t2_fuse_residual0', 6, 128, (1,), 8, 5, 'fp32', 1, 1, 2, {'fuse_residual': 0},
     [('gemm', 2, 5, 1, 4)]),
    ('k5_d128_m1_H8_td6_f16x3_B1_mode0_t2', 6, 128, (1,), 8, 5, 'f16x3', 1, 0, 2, {},
     [('gemm', 2, 5, 1, 5)]),
    ('k5_d96_m1_H8_td6_fp32_B1_mode0_t2', 6, 96, (1,), 8, 5, 'fp32', 1, 0, 2, {},
     [('gemm', 2, 5, 1, 20)]),
    ('k7_d128_m1_H8_td6_fp32_B1_mode0_t2', 6, 128, (1,), 8, 7, 'fp32', 1, 0, 2, {},
     [('gemm', 2, 7, 1, 4)]),
    ('k7_d96_m1_H8_td6_fp32_B1_mode0_t2', 6, 96, (1,), 8, 7, 'fp32', 1, 0, 2, {},
     [('gemm', 2, 7, 1, 20)]),
    ('k5_d64_m1_H200_td6_fp32_B1_mode0_t101', 6, 64, (1,), 200, 5, 'fp32', 1, 0, 101, {},
     [('gemm', 1, 5, 1, 52)]),
]
# registered kernels not reached in this space (not a claim that they are dead)
NOT_REACHED = [
    ('cc', 2, 1, 0, 1, 16, 0),
    ('cc', 2, 1, 0, 1, 32, 0),
    ('cc', 3, 2, 0, 1, 16, 0),
    ('cc', 3, 2, 0, 1, 32, 0),
    ('cc', 5, 1, 1, 1, 16, 0),
    ('cc', 5, 1, 1, 1, 32, 0),
    ('ccw', 1, 1, 0, 1, 16),
    ('ccw', 1, 1, 0, 1, 32),
    ('ccw', 2, 1, 0, 1, 16),
    ('ccw', 2, 1, 0, 1, 32),
    ('ccw', 3, 2, 0, 1, 16),
    ('ccw', 3, 2, 0, 1, 32),
    ('ccw', 5, 1, 1, 1, 16),
    ('ccw', 5, 1, 1, 1, 32),
    ('gemm', 1, 7, 1, 8),
    ('gemm', 1, 7, 1, 12),
    ('gemm', 2, 7, 1, 8),
    ('gemm', 2, 7, 1, 12),
    ('gemm', 3, 1, 1, 0),
    ('gemm', 3, 1, 1, 4),
    ('gemm', 3, 1, 1, 16),
    ('gemm', 3, 1, 1, 20),
    ('gemm', 3, 2, 1, 0),
    ('gemm', 3, 2, 1, 16),
    ('gemm', 3, 3, 1, 0),
    ('gemm', 3, 3, 1, 4),
    ('gemm', 3, 3, 1, 16),
    ('gemm', 3, 3, 1, 20),
    ('gemm', 3, 3, 2, 0),
    ('gemm', 3, 3, 2, 16),
    ('gemm', 3, 5, 1, 0),
    ('gemm', 3, 5, 1, 4),
    ('gemm', 3, 5, 1, 16),
    ('gemm', 3, 5, 1, 20),
    ('gemm', 3, 7, 1, 0),
    ('gemm', 3, 7, 1, 4),
    ('gemm', 3, 7, 1, 16),
    ('gemm', 3, 7, 1, 20),
    # not launched: the planner keeps the ride off tile 5 where these would run, because they compute wrong values (docstring)
    ('gemm', 5, 3, 1, 8),
    ('gemm', 5, 5, 1, 8),
    ('gemm', 5, 7, 1, 8),
]


# ------------------------------------------------------------------------------------------------ (a)
# What the matrix must cover besides the kernels themselves (features of tests/forward_census.py):
#   gn_pass_kernel<npt>: a windowed GroupNorm'd layer has pairs of C/8 x L elements with L >= 256 and C/8 a multiple of 4,
#   the pass holds 4 x GNP_THREADS x npt of them, npt a power of two up to 32
GN_NPT = (1, 2, 4, 8, 16, 32)
#   tiles with a grid split-K launch: every tile (a forced tile splits wherever its layer has few tiles and two K chunks)
SPLIT_TILES = tuple(range(10))
PART_TILES = tuple(range(10))
# ("big" / "ride_in", rows per tile) the planner allows: see the assertion below
SMALL_FORMS = (("big", 16), ("big", 32), ("ride_in", 16), ("ride_in", 32))


def _case_plan(case):
    """The plan of a case on an engine without weights (no device call)."""
    _, td, dim, mults, H, ks, precision, B, mode, tile, options, _ = case
    eng = census.host_engine(td, dim, mults, H, ks, precision)
    census.set_options(eng, tile, options)
    return eng.forward_plan(B, mode)


def _assert_keys(case, plan):
    have = census.plan_keys(plan)
    missing = [k for k in case[-1] if tuple(k) not in have]
    assert not missing, f"{case[0]}: the planner no longer takes this case through {missing}; it launches " \
                        f"{sorted(k for k in have if k[0] in KERNEL_FAMILIES)}"


def test_matrix_reaches_every_forward_path():
    from dynamics_aware_diffusion_amd._engine import registered_kernels
    gemm, cc, ccw = registered_kernels()
    assert (len(gemm), len(cc), len(ccw)) == (335, 18, 20)
    assert len({c[0] for c in CASES}) == len(CASES)
    reached = set()
    for case in CASES:
        plan = _case_plan(case)
        _assert_keys(case, plan)
        reached |= census.plan_keys(plan)
    kernels = {k for k in reached if k[0] in KERNEL_FAMILIES}
    listed = {tuple(k) for k in NOT_REACHED}
    assert len(listed) == len(NOT_REACHED)
    both = sorted(kernels & listed)
    assert not both, f"listed as not reached, but the matrix launches them: {both}"
    assert kernels | listed == gemm | cc | ccw, (sorted((gemm | cc | ccw) - kernels - listed), sorted((kernels | listed) - (gemm | cc | ccw)))
    # the path features
    assert {k[1] for k in reached if k[0] == "gn_npt"} == set(GN_NPT)
    for cfg in SPLIT_TILES:
        assert ("split", cfg, 1) in reached and ("split", cfg, 0) in reached, f"tile {cfg}: grid split-K on and off"
    for cfg in PART_TILES:
        assert ("part_tile", cfg) in reached, f"tile {cfg}: no launch with a partly empty last N tile"
    assert ("final_gy>1", "final_posterior_kernel") in reached and ("final_gy>1", "final_cc_kernel") in reached
    assert ("final_cc",) in reached
    assert {k[1] for k in reached if k[0] == "res_kind"} >= {1, 2, 3, 4}
    for form in SMALL_FORMS:
        assert form in reached, f"no small-batch launch with {form[0]} on {form[1]}-row tiles"


def test_forward_plan_refuses_what_its_call_refuses():
    from dynamics_aware_diffusion_amd._engine import DadError, HipEngine
    eng = HipEngine(transition_dim=6, dim=32, channels=(32, 64, 128), horizon=32, n_timesteps=T)
    for mode in (2, 3):
        with pytest.raises(DadError, match="dad_model_set_training"):
            eng.forward_plan(4, mode)
    with pytest.raises(DadError):
        eng.forward_plan(0, 0)
    with pytest.raises(DadError):
        eng.forward_plan(4, 4)
    with pytest.raises(DadError, match="too large"):
        eng.forward_plan(1 << 22, 1)
    small, rows = eng.forward_plan(4, 0), eng.forward_plan(4, 1)
    assert small["small"] and small["final"] == (4, 1, "final_cc_kernel") and len(small["launches"]) == eng.small_batch_plan(4)[0]
    assert not rows["small"] and rows["final"][2] == "final_posterior_kernel"
    assert all(q["key"][0] in ("cc", "ccw") for q in small["launches"]) and all(q["key"][0] == "gemm" for q in rows["launches"])


# ------------------------------------------------------------------------------------------------ (b)
def _inputs(name, B, H, td):
    from dynamics_aware_diffusion_amd.utils import synth
    x0 = np.clip(synth.normal_like(23, f"fpath.x.{name}", (B, H, td)) * 0.5, -1, 1).astype(np.float32)
    t = np.array([(3 * i + 1) % T for i in range(B)], dtype=np.int64)
    t[-1] = T - 1
    noise = synth.normal_like(23, f"fpath.n.{name}", (B, H, td))
    return x0, t, noise


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """Weights, inputs and the float64 oracle of a case, with the fp32 oracle's own distance; nobody writes into it."""
    from dynamics_aware_diffusion_amd.utils import synth
    from oracle import denoiser as orc
    _, td, dim, mults, H, ks, _, B, mode, _, _, _ = next(c for c in CASES if c[0] == name)
    state = synth.synth_unet_state(td, dim, mults, seed=43, affine_jitter=0.3, kernel_size=ks)
    w = as_torch(state)
    w64 = orc.cast_weights(w, torch.float64)
    x0, t, noise = _inputs(name, B, H, td)
    ref = {"state": state, "inputs": (x0, t, noise)}
    x0t, tt, nz = torch.from_numpy(x0), torch.from_numpy(t), torch.from_numpy(noise)
    if mode in (0, 1):
        if mode == 0:
            tt = torch.full((B,), 7, dtype=torch.long)
        with torch.no_grad():
            ref["out64"] = orc.unet_forward(w64, nz.double(), tt).numpy()
            ref["o_out"] = max_abs(orc.unet_forward(w, nz, tt).numpy(), ref["out64"])
        ref["t"] = tt
        return ref
    sched = orc.schedule_buffers("cosine", T)
    s64 = {k: v.double() for k, v in sched.items()}
    _, _, out64 = orc.training_loss(w64, s64, x0t.double(), tt, nz.double())
    _, _, out32 = orc.training_loss(w, sched, x0t, tt, nz)
    ref["out64"], ref["o_out"] = out64.numpy(), max_abs(out32.numpy(), out64.numpy())
    if mode == 3:
        _, g64, dx64 = orc.training_gradients(w64, s64, x0t.double(), tt, nz.double())
        _, g32, dx32 = orc.training_gradients(w, sched, x0t, tt, nz)
        scales = grad_scales(g64)
        ref["g64"], ref["dx64"], ref["scales"] = g64, dx64, scales
        ref["orc_errs"] = {k: max_abs(g32[k].numpy(), g64[k].numpy()) / scales[k] for k in g64}
        ref["orc_errs"]["d x_t"] = max_abs(dx32.numpy(), dx64.numpy()) / float(dx64.abs().max())
    return ref


def _apply(eng, tile, options, small_batch_kernels=True):
    eng.debug_set_tile(tile)
    for name, default in census.OPTION_DEFAULTS.items():
        eng.debug_set_option(name, options.get(name, int(small_batch_kernels) if name == "cc" else default))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_forward_case_vs_float64(case, dev):
    from tests.test_hip_long_horizon import _diffusion
    from tests.test_hip_train_batch import _train_step
    name, td, dim, mults, H, ks, precision, B, mode, tile, options, keys = case
    ref = _oracle(name)
    diff = _diffusion(td, td - 1, 1, dim, mults, H, T, ref["state"], dev, ks=ks, precision=precision)
    eng = diff.model.engine(H, dev, training=mode >= 2)
    x0, t, noise = ref["inputs"]
    try:
        _apply(eng, tile, options)
        _assert_keys(case, eng.forward_plan(B, mode))
        if mode in (0, 1):
            x = torch.from_numpy(noise).to(dev)
            run = (lambda: eng.unet_forward(x, 7)) if mode == 0 else (lambda: eng.unet_forward_rows(x, ref["t"].to(dev)))
            out, out2 = run().cpu().numpy(), run().cpu().numpy()
            same = np.array_equal(out, out2)
        elif mode == 2:
            x0t, tt, nz = torch.from_numpy(x0).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(noise).to(dev)
            outs = []
            for _ in range(2):
                with torch.enable_grad():
                    x_t = diff.q_sample(x0t, tt, nz).detach().requires_grad_(True)
                    outs.append(diff.model(x_t, tt).detach().cpu().numpy())
            out, same = outs[0], np.array_equal(outs[0], outs[1])
        else:
            _, out, dx, grads = _train_step(diff, x0, t, noise, dev)
            _, out2, dx2, grads2 = _train_step(diff, x0, t, noise, dev)
            same = np.array_equal(out, out2) and np.array_equal(dx, dx2) and all(np.array_equal(grads[k], grads2[k]) for k in grads)
        assert diff.model._engine is eng, "the engine was rebuilt: the plan asserted above is not the one that ran"
    finally:
        _apply(eng, -1, {}, diff.model.small_batch_kernels)
    e_out = max_abs(out, ref["out64"])
    text = f"\n{name}: output vs float64: engine {e_out:.2e}, fp32 oracle {ref['o_out']:.2e}"
    if mode == 3:
        g64, dx64, scales, orc_errs = ref["g64"], ref["dx64"], ref["scales"], ref["orc_errs"]
        assert set(grads) == set(g64)
        errs = {k: max_abs(grads[k], g64[k].numpy()) / scales[k] for k in grads}
        errs["d x_t"] = max_abs(dx, dx64.numpy()) / float(dx64.abs().max())
        worst, oworst = max(errs, key=errs.get), max(orc_errs, key=orc_errs.get)
        text += (f"; gradients vs float64, x max|g|: engine {errs[worst]:.2e} ({worst}), d x_t {errs['d x_t']:.2e}; "
                 f"fp32 oracle {orc_errs[oworst]:.2e} ({oworst}), d x_t {orc_errs['d x_t']:.2e}")
    print(text)
    assert np.isfinite(out).all()
    if mode == 3:
        for k in grads:
            assert np.isfinite(grads[k]).all(), k
        bad = {k: f"{e:.2e}" for k, e in errs.items() if not e <= REL}
        assert not bad, f"{name}: gradients farther than {REL} x max|g| from float64: {bad}"
    else:
        assert e_out <= TOL_STEP, f"{name}: output {e_out:.2e} from the float64 forward (the fp32 oracle: {ref['o_out']:.2e})"
    assert same, f"{name}: a second call gives other bits"
