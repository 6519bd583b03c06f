"""The cases of tests/test_gpu_graph_replay.py (a plain module: importable without a GPU, no torch).

One case per kernel family of sow_amd/csrc: the smallest shape that still selects the family (the predicates of api.hip
as tests/fuzz_plan.py mirrors them, the shapes of the tables in tests/test_gpu_elementwise.py, fused_acc_numerics.py,
deep_acc_numerics.py, shared_fused_acc_numerics.py, test_gpu_skinny.py, test_gpu_tt_elementwise.py and
test_gpu_step_elementwise.py).  A case is captured into a HIP graph and replayed in place by tests/graph_replay.py.

`claims` of a case: the __global__ kernels its eager run has to show in the profiler's trace (test_zz_graph_coverage).
Coverage condition (tests/test_graph_plan_cpu.py): every __global__ name of sow_amd/csrc/*.hip and *.hpp -- `kernel_names`
reads the sources for names only -- is claimed by at least one case or stands in EXEMPT with a reason that points at a
host read in the documented contract of the kernel's entry point.
"""
from __future__ import annotations

import dataclasses
import os
import re
from typing import Dict, List, Tuple

import fuzz_plan as FP

L = FP.Layer


@dataclasses.dataclass
class Case:
    id: str
    kind: str                   # the builder of tests/test_gpu_graph_replay.py
    p: dict                     # the builder's parameters
    claims: Tuple[str, ...]     # kernels the eager twin's trace must show
    shape: Tuple[int, ...]      # the numbers the id has to name
    cost: float                 # multiply-adds of the float64 reference of ONE input set


# Kernels no case claims: name -> the host read in the entry point's documented contract that keeps it out of a capture.
# Every kernel of the library sits behind a C entry point that takes a stream and reads nothing back (ops.absmax's .item()
# belongs to the Python wrapper; sow_absmax itself is captured below), so the dict is empty.
EXEMPT: Dict[str, str] = {}


# ---- the __global__ names of the sources ----------------------------------------------------------------------------------
_GLOBAL = re.compile(r"__global__(?:\s+__launch_bounds__\([^)]*\))?\s+void\s+(\w+)\s*\(")


def kernel_names(csrc: str = None) -> set:
    """The names of the __global__ functions of csrc/*.hip and *.hpp.  A kernel whose name is a macro (gemm4_body.hpp is
    included once per dtype) counts under every value the sources #define for that macro."""
    csrc = csrc or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sow_amd", "csrc")
    names, defines = set(), {}
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".hpp")):
            continue
        with open(os.path.join(csrc, fn)) as f:
            text = f.read()
        names.update(_GLOBAL.findall(text))
        for m in re.finditer(r"^\s*#\s*define\s+(\w+)\s+(\w+)\s*$", text, re.M):
            defines.setdefault(m.group(1), set()).add(m.group(2))
    out = set()
    for n in names:
        out.update(defines.get(n, {n}))
    return out


# ---- layers: sow_forward + sow_backward_ex ----------------------------------------------------------------------------------
def _layer(tag, lay: FP.Layer, claims, flags=None, param_f32=False, check="elementwise"):
    lay.name = FP._name(lay, tag) + (f"_{flags}" if flags else "") + ("_paramf32" if param_f32 else "")
    if lay.acc == "lowrank" and not flags:
        lay.y_rounds = lay.dx_rounds = "twice"
    cost = FP.ref_cost(lay)
    return Case("layer_" + lay.name, "layer", dict(layer=lay, flags=flags, param_f32=param_f32, check=check), tuple(claims),
                (lay.T, lay.d_in, lay.d_out, lay.r) + ((lay.r_acc,) if lay.r_acc else ()), cost)


LAYERS = [
    # chain2 streaming (T / 64 > 128 token blocks, widths % 8, r even in [4, 64]) + the wide LDS-DMA weight-gradient kernel
    _layer("chain2", L("", "bf16", 8193, 64, 128, 16, s=0.5, grad_beta=1.0),
           ("chain2_kernel", "tn_partial_dma_wide_kernel", "tn_reduce_kernel")),
    _layer("chain2", L("", "f16", 8193, 128, 64, 16, bias=False), ("chain2_f16_kernel", "tn_partial_dma_wide_kernel")),
    # r = 64 with a bias: no free ones column, dbias by colsum_kernel
    _layer("chain2_r64", L("", "bf16", 8193, 64, 128, 64), ("chain2_kernel", "colsum_kernel")),
    # TN_NARROW: the narrow LDS-DMA weight-gradient kernel
    _layer("chain2", L("", "bf16", 8193, 72, 136, 8, s=2.0, switches={"TN_NARROW": 1}), ("tn_partial_dma_kernel",)),
    # fp32 parameters (SOW_PARAM_F32): packed into the workspace at every call
    _layer("chain2", L("", "bf16", 8193, 64, 128, 16, s=0.5), ("pack_params_kernel", "chain2_kernel"), param_f32=True,
           check="param_f32"),
    # the short split: T / 64 <= 128 token blocks and >= 24 column tiles: phase 1 over K + h_reduce, phase 2 over columns
    _layer("short", L("", "bf16", 64, 640, 960, 16, s=0.5), ("chain2_kernel", "h_reduce_kernel")),
    _layer("short", L("", "f32", 64, 640, 960, 16, bias=False), ("chain2f_kernel", "h_reduce_kernel")),
    # generic chain and weight-gradient kernels: odd rank, widths off 8
    _layer("generic", L("", "bf16", 193, 77, 100, 3, s=0.5, grad_beta=0.5), ("chain_kernel", "tn_partial_kernel")),
    _layer("generic", L("", "f16", 63, 72, 100, 2), ("chain_kernel", "tn_partial_kernel")),
    _layer("generic", L("", "f32", 193, 77, 100, 1, bias=False), ("chain_kernel", "tn_partial_kernel")),
    # dense accumulator, r <= 64: gemm4h (<= 2 column tiles of 256 both ways, >= 120 tiles)
    _layer("gemm4h", L("", "bf16", 60 * 256 + 1, 264, 264, 16, acc="dense", s=0.5), ("gemm4_kernel",)),
    _layer("gemm4h", L("", "f16", 60 * 256 + 1, 264, 264, 16, acc="dense", bias=False), ("gemm4_f16_kernel",)),
    # gemm2h: gemm4h switched off, >= 160 tiles of 256 x 256
    _layer("gemm2h", L("", "bf16", 80 * 256 + 1, 264, 264, 16, acc="dense", switches={"NO_GEMM4H": 1}), ("gemm2h_kernel",)),
    # d_out > 512 at short T: H-only chain pass (split over K), then the dense product with the rank extension split over K
    # through the workspace; the data gradient (K = 2048) takes gemm3s with A padded to 64 columns by pad64_kernel
    _layer("splitk", L("", "bf16", 1024, 6144, 2048, 16, acc="dense", s=0.5),
           ("gemm4_kernel", "gemm4_splitk_reduce_kernel", "pad64_kernel", "gemm3s_kernel", "h_reduce_kernel")),
    # r in (64, 256]: the fused wide chain, its pack launch and the token-slab weight-gradient kernel (two slabs)
    _layer("wide", L("", "bf16", 601, 72, 136, 96, s=0.5),
           ("chain_wide_kernel", "wide_pack_kernel", "tnw_partial_kernel", "tnw_reduce_kernel")),
    _layer("wide", L("", "f16", 601, 136, 72, 66, bias=False, acc="lowrank", r_acc=70), ("chain_wide_kernel", "wide_pack_kernel")),
    # ragged widths; with a dense accumulator its product runs on gemm_rag
    _layer("ragged", L("", "f16", 601, 77, 139, 96, s=0.5), ("chain_wide_kernel", "tnw_partial_kernel")),
    _layer("ragged", L("", "bf16", 601, 77, 136, 66, acc="dense", y_rounds="twice", dx_rounds="twice"), ("gemm_rag_kernel",)),
    # fp32: chain3f + its planes pre-pass (T >= 8192), the quad weight-gradient kernel (T >= 4096, >= 3 column groups)
    _layer("chain3f", L("", "f32", 8193, 256, 264, 16, s=0.5),
           ("chain3f_kernel", "chain3f_planes_kernel", "tn_partial_f32_quad_kernel")),
    # chain2f below 8192 tokens; fewer than 3 column groups: the wide fp32 weight-gradient kernel, TN_NARROW: the narrow one
    _layer("chain2f", L("", "f32", 1000, 128, 128, 16), ("chain2f_kernel", "tn_partial_dma_f32_wide_kernel")),
    _layer("chain2f", L("", "f32", 1000, 128, 128, 16, s=0.5, switches={"TN_NARROW": 1}), ("tn_partial_dma_f32_kernel",)),
    # the fused low-rank-accumulator passes (fused_acc_numerics.CASES[0], deep_acc_numerics "tot258")
    _layer("fused", L("", "bf16", 193, 72, 264, 50, acc="lowrank", r_acc=50, s=0.75),
           ("chain_wide_acc_kernel", "wide_acc_pack_kernel"), flags="FUSE_ACC", check="fused"),
    _layer("deep", L("", "bf16", 193, 72, 264, 58, acc="lowrank", r_acc=200, s=0.75),
           ("chain_deep_acc_kernel", "wide_acc_pack_kernel"), flags="FUSE_ACC_DEEP", check="fused"),
]


# ---- grouped, deferred, shared ------------------------------------------------------------------------------------------------
def _group(tag, dtype, T, widths, deferred, rows, claims):
    layers = [L(f"g{i}", dtype, T, d_in, d_out, r, bias=bias, s=s, seed=i) for i, (d_in, d_out, r, bias, s) in enumerate(widths)]
    cid = f"group_{tag}_{dtype}_T{T}_" + "_".join(f"{c.d_in}x{c.d_out}r{c.r}" for c in layers)
    return Case(cid, "group", dict(layers=layers, deferred=deferred, rows=rows, dtype=dtype), tuple(claims),
                (T,) + tuple(v for c in layers for v in (c.d_in, c.d_out, c.r)), sum(FP.ref_cost(c) for c in layers))


GROUPS = [
    # four layers of a block: the row-owner plan (tn_rows_plan: 160 .. 256 slab ranges of >= 512 tokens over the group)
    _group("rows", "bf16", 16385, [(256, 256, 16, True, 0.5), (256, 256, 8, False, 1.0), (256, 256, 50, True, 2.0),
                                   (256, 256, 62, False, 0.5)], False, True, ("tn_partial_rows_kernel", "chain2_kernel")),
    # BWD_WEIGHTS_PARTIAL | BWD_GROUP_SLABS, then every reduction in one sow_reduce_batch launch
    _group("deferred", "bf16", 8193, [(64, 128, 16, True, 0.5), (64, 72, 8, False, 1.0), (128, 64, 4, True, 2.0)], True, False,
           ("tn_reduce_batch_kernel", "tn_partial_dma_wide_kernel")),
]

SHARED = [
    Case("shared_bf16_T8193_in64_64r16_128r8", "shared",
         dict(dtype="bf16", T=8193, d_in=64, sibs=[(64, 16, False, 0.5), (128, 8, True, 1.0)], grad_beta=1.0),
         ("chain2_shared_kernel",), (8193, 64, 64, 16, 128, 8), 2 * 14.0 * 8193 * (64 + 128) * 64),
    # shared_fused_acc_numerics.CASES "four_tiny_beta": four siblings with a low-rank accumulator, grad_beta = 1
    Case("shared_acc_bf16_T8193_in8_4x24r2acc2", "shared_acc", dict(case="four_tiny_beta"),
         ("chain_shared_acc_kernel", "shared_acc_pack_kernel"), (8193, 8, 4, 24, 2, 2), 4 * 24.0 * 8193 * (8 + 24) * 64),
]

SKINNY = [
    Case("skinny_bf16_T17_520x264_r8_dense", "skinny", dict(dtype="bf16", T=17, d_in=520, d_out=264, r=8, bias=True, s=1.0,
                                                            acc="dense"),
         ("skinny_a_kernel", "skinny_b_kernel"), (17, 520, 264, 8), 3.0 * 17 * 520 * 264),
    Case("skinny_f16_T32_264x520_r2", "skinny", dict(dtype="f16", T=32, d_in=264, d_out=520, r=2, bias=True, s=1.0, acc="none"),
         ("skinny_a_kernel", "skinny_b_kernel"), (32, 264, 520, 2), 3.0 * 32 * 520 * 64),
]


# ---- sow_gemm_ex ------------------------------------------------------------------------------------------------------------------
def _gemm(dtype, M, N, K, claims, use_ws=False, switches=None, beta=0.0, bias=True):
    cid = (f"gemm_{dtype}_{M}x{N}x{K}" + ("_ws" if use_ws else "") + (f"_b{beta:g}" if beta else "")
           + "".join(f"_{k}{v}" for k, v in (switches or {}).items()))
    return Case(cid, "gemm", dict(dtype=dtype, M=M, N=N, K=K, use_ws=use_ws, switches=dict(switches or {}), beta=beta, bias=bias),
                tuple(claims), (M, N, K), 2.0 * M * N * K)


GEMMS = [
    _gemm("bf16", 5120, 1536, 512, ("gemm4_kernel",)),                        # 120 tiles of 256 x 256, no workspace
    _gemm("bf16", 1024, 2048, 6144, ("gemm4_kernel", "gemm4_splitk_reduce_kernel"), use_ws=True, bias=False),
    _gemm("f16", 1024, 2048, 6144, ("gemm4_f16_kernel", "gemm4_f16_splitk_reduce_kernel"), use_ws=True, beta=1.0),
    _gemm("bf16", 1536, 1024, 512, ("gemm3s_kernel",), beta=1.0),              # 96 tiles of 128 x 128, K = 512
    _gemm("bf16", 1536, 1024, 512, ("gemm2_kernel",), switches={"GEMM3S": 0}),
    _gemm("bf16", 1536, 1024, 512, ("gemm3_kernel",), switches={"GEMM3S": 0, "GEMM3": 1}),
    _gemm("bf16", 130, 77, 50, ("gemm_kernel",)),                              # N off 8: the generic kernel
    _gemm("f32", 256, 132, 64, ("gemm_x3_kernel",), beta=1.0),
]


# ---- flat optimizer kernels -------------------------------------------------------------------------------------------------------
def _small(cid, kind, p, claims, shape, cost=0.0):
    return Case(cid, kind, p, tuple(claims), tuple(shape), cost)


N_FLAT = 2048 * 256 + 12345      # past the 2048-block grid of the flat kernels, not a multiple of 256
OPTIM = [
    _small(f"adamw_flat_bf16_f32_n{N_FLAT}", "adamw_flat", dict(pdtype="bf16", sdtype="f32", n=N_FLAT, step=7),
           ("adamw_flat_kernel",), (N_FLAT,)),
    _small("adamw_flat_seg_f16_f16_300_1000_777", "adamw_seg", dict(pdtype="f16", sdtype="f16", lens=(300, 1000, 777)),
           ("adamw_flat_seg_kernel",), (300, 1000, 777)),
    _small("adamw_flat_seg_stats_bf16_f32_300_1000_777", "adamw_seg_stats", dict(pdtype="bf16", sdtype="f32", lens=(300, 1000, 777)),
           ("grad_sumsq_partial_kernel", "grad_stats_finalize_kernel", "adamw_flat_seg_stats_kernel"), (300, 1000, 777)),
    _small("grad_stats_flat_f32_n70001", "grad_stats", dict(dtype="f32", n=70001),
           ("grad_sumsq_partial_kernel", "grad_stats_finalize_kernel"), (70001,)),
    _small("zero_state_60_spans", "zero", dict(spans=60), ("multi_zero_kernel",), (60,)),
]

# ---- tensor-train kernels and the small helpers ---------------------------------------------------------------------------------------
TT = [
    _small("tt_reconstruct_o2r3_o3r16", "tt_reconstruct", dict(specs=("o2_r3", "o3_r16")), ("tt_reconstruct_kernel",), (2, 3, 3, 16),
           4.0e7),
    _small("tt_decompose_o2r16_o3r9_o1", "tt_decompose", dict(specs=("o2_r16", "o3_r9", "o1")),
           ("tt_pad_interleave_kernel", "tt_stage_copy_in_kernel", "qr_panel_batch_kernel", "tt_stage_copy_out_kernel",
            "tt_stage_rrest_kernel"), (2, 16, 3, 9, 1), 1.0e8),
    _small("ttadam_batch_o2r16_state_o4r4_nostate", "ttadam_batch", dict(items=(("o2_r16", 1), ("o4_r4", 0))),
           ("tt_adam_eval_kernel", "tt_stage_copy_in_kernel", "qr_panel_batch_kernel", "tt_stage_copy_out_kernel"), (2, 16, 4, 4), 1.0e8),
    _small(f"ttadam_dense_n{N_FLAT}", "ttadam_dense", dict(n=N_FLAT), ("ttadam_dense_kernel",), (N_FLAT,)),
    _small("tt_kron_core_3x5_28_6x9", "kron", dict(ra0=3, rb0=5, ij=28, ra1=6, rb1=9), ("tt_kron_core_kernel",), (3, 5, 28, 6, 9)),
    _small("small_inverse_b1000_r7", "inverse", dict(batch=1000, r=7), ("small_inverse_kernel",), (1000, 7)),
    _small("absmax_n100003", "absmax", dict(n=100003), ("absmax_kernel",), (100003,)),
    _small("axpby_bf16_n524365", "axpby", dict(dtype="bf16", n=2048 * 256 + 77), ("axpby_kernel",), (524365,)),
    _small("cast_copy_flat_f32_bf16_n70005", "cast", dict(src="f32", dst="bf16", n=70005, strided=False), ("cast_flat_kernel",),
           (70005,)),
    _small("cast_copy_strided_f16_f32_543x129", "cast", dict(src="f16", dst="f32", rows=543, cols=129, strided=True),
           ("cast_copy_kernel",), (543, 129)),
]

# ---- QR and accumulate -----------------------------------------------------------------------------------------------------------------
QR = [
    _small("qr_thin_panel_f32_bf16_259x100_k50", "qr", dict(m=259, n=100, k=50, din="f32", dout="bf16", need_r=1, extra_ld=2),
           ("qr_copy_in_kernel", "qr_panel_kernel", "qr_copy_out_kernel"), (259, 100, 50), 4.0 * 259 * 100 * 100),
    _small("qr_thin_blocked_bf16_f32_300x200_k200", "qr", dict(m=300, n=200, k=200, din="bf16", dout="f32", need_r=1, extra_ld=0),
           ("qr_copy_in_kernel", "qr_block_panel_kernel", "qr_larfb_kernel", "qr_eye_kernel", "qr_copy_out_kernel"), (300, 200, 200),
           4.0 * 300 * 200 * 200),
    _small("accumulate_batch_bf16_6_items_100x259", "accumulate", dict(dtype="bf16", items=6),
           ("rank_update_batch_kernel", "qr_copy_in_batch_kernel", "qr_panel_batch_kernel", "qr_copy_out_batch_kernel"),
           (6, 100, 259), 6 * 4.0 * 259 * 100 * 64),
]

CASES: List[Case] = LAYERS + GROUPS + SHARED + SKINNY + GEMMS + OPTIM + TT + QR


def claimed() -> set:
    return {k for c in CASES for k in c.claims}
