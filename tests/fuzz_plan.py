"""The seeded random sweep of tests/test_gpu_fuzz_elementwise.py (a plain module: importable without a GPU, no torch).

`plan(seed)` draws every case of the sweep, deterministically:
* layers: one stratum per dispatch family of sow_forward / sow_backward_ex, each case carrying its shape and settings, the
  kernel family it targets (read off the *_supported / *_shape_ok predicates and the dispatch of api.hip, mirrored below)
  and the rounding class of y and of dX ("once" | "twice", include/sow_amd.h and tests/test_gpu_elementwise.py);
* groups: sets of 2 - 4 layers through sow_forward_group / sow_backward_group, a share with the deferred reduction;
* shared: sibling sets inside chain2_shared_supported;
* gemms: sow_gemm_ex in bf16 / f16 / fp32, every transpose combination, strided operands.
A second stream (seed + 1, drawn after the four lists above, which it leaves what they were) covers the families that landed
after the first sweep:
* skinny / skinny_groups: sow_forward_skinny per accumulator kind, every slab length, tail and column class of skinny_plan
  (mirrored below), odd ranks, grouped calls whose layers differ in T, d_in and slab length;
* fused / deep: SOW_FUSE_ACC and SOW_FUSE_ACC_DEEP layers over every r_pad; shared_acc: sibling sets of
  sow_backward_shared | SOW_FUSE_ACC inside the LDS rule, one exactly at it;
* eight ragged layers with a dense accumulator (gemm_rag_kernel), appended to `layers`.

Every case's id names its shape, so that a failure names its case.  `ref_cost` is the float64 reference work of a case
(multiply-adds of the CPU products of the checks); the CPU test keeps every case under REF_COST_CAP.
"""
from __future__ import annotations

import dataclasses
import random
from typing import List, Optional

SEED = 20261016
REF_COST_CAP = 6.0e10          # multiply-adds of one case's float64 reference
LAYER_SWITCHES = ("NO_GEMM4H", "GEMM4", "GEMM3S", "NO_SPLITK", "NO_WIDE_CHAIN", "NO_RAGGED", "F32_EXACT", "FORCE_CHAIN_V1",
                  "NO_CHAIN3F", "NO_TN_F32Q", "TN_NARROW", "NO_RAGGED_GEMM")

# the kernel families the sweep has to reach (test_zz_fuzz_coverage); "chain_wide_kernel" is counted apart for aligned and
# ragged widths, gemm4_kernel as plain, h-fused and split-K.  FAMILIES_FIRST: those of the first stream, which the chosen-value
# cases of tests/value_plan.py are taken from; FAMILIES adds those of the second (skinny_a_kernel per accumulator format and
# with fp32 factors)
FAMILIES_SECOND = ("skinny_a_kernel[plain]", "skinny_a_kernel[e4m3]", "skinny_a_kernel[mxfp4]", "skinny_a_kernel[fp32-factors]",
                   "skinny_b_kernel", "chain_wide_acc_kernel", "chain_deep_acc_kernel", "chain_shared_acc_kernel", "gemm_rag_kernel")
FAMILIES_FIRST = ("chain2_kernel", "chain2_f16_kernel", "h_reduce_kernel", "chain_kernel", "chain_wide_kernel[aligned]",
            "chain_wide_kernel[ragged]", "chain3f_kernel", "chain2f_kernel", "chain2_shared_kernel",
            "tn_partial_dma_kernel|tn_partial_dma_wide_kernel", "tn_partial_rows_kernel", "tn_partial_kernel",
            "tnw_partial_kernel", "tn_partial_f32_quad_kernel", "tn_partial_dma_f32_kernel|tn_partial_dma_f32_wide_kernel",
            "colsum_kernel", "gemm4_kernel[plain]", "gemm4_kernel[h]", "gemm4_kernel[splitk]", "gemm4_f16_kernel",
            "gemm2h_kernel", "gemm2_kernel", "gemm3s_kernel", "gemm_x3_kernel", "gemm_kernel")
FAMILIES = FAMILIES_FIRST + FAMILIES_SECOND


@dataclasses.dataclass
class Layer:
    name: str
    dtype: str                  # "bf16" | "f16" | "f32"
    T: int
    d_in: int
    d_out: int
    r: int
    acc: Optional[str] = None   # None | "dense" | "lowrank"
    r_acc: int = 0
    bias: bool = True
    s: float = 1.0
    grad_beta: float = 0.0
    misalign: int = 0
    switches: dict = dataclasses.field(default_factory=dict)
    save_h: bool = True
    seed: int = 0
    stratum: str = ""
    family: str = ""            # kernel that must appear in the trace of the forward + backward
    y_rounds: str = "once"
    dx_rounds: str = "once"
    edges: tuple = ()           # named edges this case draws ("c3f_dout_mod4", "rag_in_5", "slab+1", ...)


@dataclasses.dataclass
class Group:
    name: str
    layers: List[Layer]
    deferred: bool              # BWD_WEIGHTS_PARTIAL + sow_backward_group_reduce_desc + sow_reduce_batch
    rows: bool                  # tn_rows_plan of the set (the C plan is asserted against the trace)


@dataclasses.dataclass
class Sib:
    d_out: int
    r: int
    bias: bool
    s: float


@dataclasses.dataclass
class Shared:
    name: str
    dtype: str
    T: int
    d_in: int
    sibs: List[Sib]
    grad_beta: float


@dataclasses.dataclass
class Gemm:
    name: str
    dtype: str
    M: int
    N: int
    K: int
    trans_a: bool
    trans_b: bool
    lda: int
    ldb: int
    ldc: int
    alpha: float
    beta: float
    bias: bool
    use_ws: bool
    switches: dict
    family: str
    seed: int


# ---- mirrors of the C planning functions ------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def tnw_pick_slabs(T, d_in, d_out):
    """skinny_tn_wide.hip: (slab count, slab length)."""
    tiles = cdiv(d_in, 64) + cdiv(d_out, 64)
    ns = cdiv(512, tiles)
    ns = min(ns, max(T // 256, 1), 64)
    ns = max(ns, 1)
    ln = cdiv(cdiv(T, ns), 64) * 64
    ln = max(ln, 64)
    return cdiv(T, ln), ln


def tn_rows_plan(Ts, Ds):
    """skinny_tn.hip tn_rows_plan (the workspace cap never binds: plan_ws sizes it for T / 512 slabs up to 40)."""
    if not Ts or len(Ts) > 16 or any(d % 8 for d in Ds):
        return False
    work = sum(t * d for t, d in zip(Ts, Ds))
    total = 0
    for t, d in zip(Ts, Ds):
        nr = cdiv(cdiv(d, 64), 16)
        ns = int(256.0 * t * d / work) // nr
        ns = max(min(ns, max(t // 512, 1)), 1)
        if ns > 40:
            return False
        ln = cdiv(cdiv(t, ns), 32) * 32
        ns = cdiv(t, ln)
        total += ns * nr
    return 160 <= total <= 256


def ref_cost(c) -> float:
    """Multiply-adds of the float64 products a case's checks form on the CPU."""
    if isinstance(c, Layer):
        rr = max(c.r, 64)
        cost = 14.0 * c.T * (c.d_in + c.d_out) * rr
        if c.acc == "dense":
            cost += 4.0 * c.T * c.d_in * c.d_out
        elif c.acc == "lowrank":
            cost += 10.0 * c.T * (c.d_in + c.d_out) * c.r_acc
        return cost
    if isinstance(c, Group):
        return sum(ref_cost(m) for m in c.layers)
    if isinstance(c, Shared):
        return sum(14.0 * c.T * (c.d_in + sb.d_out) * 64 for sb in c.sibs)
    if isinstance(c, Skinny):       # x W and its squares once (the tie-clearing step keeps them), x A and h B per pass of it
        return (2.0 * c.T * c.d_in * c.d_out if c.kind != "none" else 0.0) + 16.0 * c.T * (c.d_in + c.d_out) * 64
    if isinstance(c, SkinnyGroup):
        return sum(ref_cost(m) for m in c.layers)
    if isinstance(c, Fused):        # fused_acc_numerics.check: the products over r_pad columns, forward and backward
        return 14.0 * c.T * (c.d_in + c.d_out) * (64 + r_pad(c.r + c.r_acc))
    if isinstance(c, SharedAcc):
        return sum(6.0 * c.T * (c.d_in + sb.d_out) * r_pad(sb.r + sb.r_acc) for sb in c.sibs)   # shared_fused_acc_numerics.dx_reference
    return 2.0 * c.M * c.N * c.K


# ---- the draw -------------------------------------------------------------------------------------------------------
class _Draw:
    def __init__(self, seed):
        self.g = random.Random(seed)
        self.n = 0

    def m8(self, lo, hi):
        return 8 * self.g.randint(cdiv(lo, 8), hi // 8)

    def even(self, lo, hi):
        return 2 * self.g.randint(cdiv(lo, 2), hi // 2)

    def settings(self, c: Layer, h_null_ok=True):
        g = self.g
        c.bias = g.random() < 0.6
        c.s = g.choice([1.0, 0.5, 1.0 / c.r, 2.0])
        c.grad_beta = g.choice([0.0, 0.0, 0.5, 1.0])
        c.seed = self.n
        self.n += 1
        if h_null_ok and c.acc is None and g.random() < 0.12:
            c.save_h = False
        return c


def _name(c: Layer, tag):
    parts = [tag, c.dtype, f"T{c.T}", f"{c.d_in}x{c.d_out}", f"r{c.r}"]
    if c.acc:
        parts.append(f"{c.acc}{c.r_acc or ''}")
    if c.misalign:
        parts.append("mis")
    if not c.save_h:
        parts.append("noh")
    for k, v in c.switches.items():
        parts.append(f"{k}{v}")
    return "_".join(parts)


def _finish(c: Layer, tag):
    if c.acc == "lowrank":
        c.y_rounds = c.dx_rounds = "twice"
    c.name = _name(c, tag)
    return c


def _wide_T(g, d_in, d_out, kind):
    """T of a wide-rank layer by kind: below 64, below 256, or one past / one short of a slab boundary of tnw_pick_slabs."""
    if kind == "T<64":
        return g.randint(1, 63)
    if kind == "T<256":
        return g.randint(64, 255)
    ns_lo = 2
    for _ in range(10000):
        T = g.randint(600, 8300)
        ns, ln = tnw_pick_slabs(T, d_in, d_out)
        if ns >= ns_lo and ((kind == "slab+1" and T % ln == 1) or (kind == "slab-1" and T % ln == ln - 1)):
            return T
    raise AssertionError("no slab boundary found")


def _layers(d: _Draw) -> List[Layer]:
    g = d.g
    out: List[Layer] = []

    def add(c, tag, switch=None, h_null_ok=True):
        d.settings(c, h_null_ok)
        if switch:
            c.switches = dict(switch)
        out.append(_finish(c, tag))
        return c

    # ---------------------------------------------------------------- bf16 / f16, r <= 64, aligned
    for i in range(8):   # chain2 streaming: T / 64 > SHORT_NTB = 128 token blocks, widths % 8, r even in [4, 64]
        dt = "bf16" if i % 2 == 0 else "f16"
        c = Layer("", dt, g.randint(8193, 20000), d.m8(64, 520), d.m8(64, 520), d.even(4, 64), stratum="chain2",
                  family="chain2_kernel" if dt == "bf16" else "chain2_f16_kernel")
        sw = None
        if i == 2:
            sw, c.family = {"TN_NARROW": 1}, "tn_partial_dma_kernel"
        elif i == 5:
            sw, c.family = {"FORCE_CHAIN_V1": 1}, "chain_kernel"
        elif i == 6:
            c.r = 64   # r = 64 with a bias: dbias by colsum_kernel
        add(c, "chain2", sw)
        if i == 6:
            c.bias = True
            c.name = _name(c, "chain2")
    for i in range(7):   # the short split: T / 64 <= 128 token blocks, >= 24 column tiles: chain2 K-split + h_reduce
        dt = "bf16" if i % 2 == 0 else "f16"
        T = g.choice([64, 65, 127, g.randint(200, 1000), g.randint(1000, 4000), 8192])
        d_in = d.m8(640, 1536)
        need = max(24 * 64 - d_in, 64)
        c = Layer("", dt, T, d_in, d.m8(need + 64, need + 512), d.even(4, 64), stratum="short",
                  family="h_reduce_kernel")
        sw = {"FORCE_CHAIN_V1": 1} if i == 4 else None
        if sw:
            c.family = "chain_kernel"
        add(c, "short", sw, h_null_ok=False)
    for i in range(5):   # gemm4h: dense accumulator, <= 2 column tiles of 256 both ways, >= 120 tiles
        dt = "bf16" if i % 2 == 0 else "f16"
        d_out, d_in = d.m8(264, 512), d.m8(264, 512)
        T = g.randint(60 * 256 + 1, 64 * 256)
        c = Layer("", dt, T, d_in, d_out, d.even(2, 64), acc="dense", stratum="gemm4h",
                  family="gemm4_kernel" if dt == "bf16" else "gemm4_f16_kernel")
        add(c, "gemm4h", h_null_ok=False)
    for i in range(3):   # gemm2h: gemm4h switched off, >= 160 tiles of 256 x 256 (two column tiles)
        d_out, d_in = d.m8(264, 512), d.m8(264, 400)
        c = Layer("", "bf16", g.randint(80 * 256 + 1, 84 * 256), d_in, d_out, d.even(4, 64), acc="dense",
                  stratum="gemm2h", family="gemm2h_kernel")
        add(c, "gemm2h", {"NO_GEMM4H": 1} if i != 1 else {"GEMM4": 0}, h_null_ok=False)
    # dense d_out > 512 at short T: chain2 H-only pass, then the dense product with the rank extension in one accumulator
    for i in range(3):   # split over K: <= 128 output tiles, >= 96 K-tiles of 64 (d_in >= 6080), tiles x splits >= 120; the bf16 gate of pick_gemm
        # wants >= 96 tiles of 128 x 128, so d_out >= 2048 at T = 1024
        c = Layer("", "bf16", g.choice([1024, 1025]), g.choice([6144, 6152]), g.choice([2048, 2056]),
                  d.even(4, 64), acc="dense", stratum="dense_short", family="gemm4_splitk_reduce_kernel")
        sw = {"NO_SPLITK": 1} if i == 2 else None
        if sw:
            c.family = "gemm3s_kernel"
        add(c, "splitk", sw, h_null_ok=False)
    for i in range(4):   # gemm3s: < 160 tiles of 256, >= 96 of 128, K >= 512; GEMM3S = 0 takes gemm2_kernel (K < 2048)
        c = Layer("", "bf16", g.randint(1536, 2100), d.m8(520, 1536), d.m8(1544, 2048), d.even(4, 64), acc="dense",
                  stratum="dense_short", family="gemm3s_kernel")
        sw = None
        if i >= 2:
            sw, c.family = {"GEMM3S": 0}, "gemm2_kernel"
        add(c, "dense_short", sw, h_null_ok=False)
        # the backward's dY W^T (N = d_in, K = d_out) takes the fused gemm2 form only where the bf16 gate of pick_gemm admits it
        c.dx_rounds = "once" if gemm2_ok(c.T, c.d_in, c.d_out) else "twice"
    for i in range(3):   # gemm2_kernel at long T: >= 160 big tiles with gemm4 switched off, K < 2048
        # (d_in > 128: the backward's dY W^T then has >= 96 tiles of 128 x 128 and takes the fused gemm2 form too)
        c = Layer("", "bf16", g.randint(8193, 10240), d.m8(136, 256), d.m8(1032, 1280), d.even(4, 64), acc="dense",
                  stratum="dense_long", family="gemm2_kernel")
        add(c, "dense_gemm2", {"GEMM4": 0}, h_null_ok=False)
    for i in range(2):   # f16 dense at short T: gemm4_f16 (plain) / the generic GEMM, then the chain with beta = 1
        c = Layer("", "f16", g.randint(1536, 2100), d.m8(520, 1024), d.m8(1544, 2048), d.even(4, 64), acc="dense",
                  stratum="dense_short", family="gemm_kernel", y_rounds="twice", dx_rounds="twice")
        add(c, "dense_f16", h_null_ok=False)
    for i in range(6):   # low-rank accumulators with r_acc on both sides of 64
        dt = "bf16" if i % 2 == 0 else "f16"
        r_acc = d.even(4, 64) if i < 3 else d.even(66, 200)
        c = Layer("", dt, g.randint(8193, 12000), d.m8(64, 400), d.m8(64, 400), d.even(4, 64), acc="lowrank", r_acc=r_acc,
                  stratum="lowrank")
        c.family = ("chain2_kernel" if dt == "bf16" else "chain2_f16_kernel") if r_acc <= 64 else "chain_wide_kernel"
        add(c, "lowrank", h_null_ok=False)

    # ---------------------------------------------------------------- bf16 / f16, even r in (64, 256]
    def wide_T(d_in, d_out, kind):
        return _wide_T(g, d_in, d_out, kind)

    kinds = ("T<64", "T<256", "slab+1", "slab-1")
    for i in range(12):   # aligned widths
        dt = "bf16" if i % 2 == 0 else "f16"
        d_in, d_out = d.m8(64, 600), d.m8(64, 600)
        kind = kinds[i % 4]
        c = Layer("", dt, wide_T(d_in, d_out, kind), d_in, d_out, d.even(66, 256), stratum="wide",
                  family="chain_wide_kernel", edges=(kind,))
        if i in (4, 5, 9):
            c.acc, c.r_acc = "lowrank", (d.even(2, 64) if i == 4 else d.even(66, 256))
        elif i in (6, 7):
            c.acc, c.y_rounds, c.dx_rounds = "dense", "twice", "twice"
        sw = None
        if i == 10:
            sw, c.family = {"NO_WIDE_CHAIN": 1}, "gemm_kernel"
        add(c, "wide", sw)
    for i in range(14):   # ragged widths: every residue 1 .. 7 (mod 8) of d_in and of d_out
        dt = "bf16" if i % 2 == 0 else "f16"
        res = i % 7 + 1
        rag = 8 * g.randint(8, 70) + res
        other = d.m8(64, 560) if g.random() < 0.6 else 8 * g.randint(8, 70) + g.randint(1, 7)
        d_in, d_out = (rag, other) if i < 7 else (other, rag)
        kind = kinds[i % 4]
        c = Layer("", dt, wide_T(d_in, d_out, kind), d_in, d_out, d.even(66, 256), stratum="ragged",
                  family="chain_wide_kernel",
                  edges=(kind, f"rag_{'in' if i < 7 else 'out'}_{res}") + ((f"rag_in_{d_in % 8}",) if i >= 7 and d_in % 8 else ())
                  + ((f"rag_out_{d_out % 8}",) if i < 7 and d_out % 8 else ()))
        if i in (3, 8, 12):
            c.acc, c.r_acc = "lowrank", d.even(2, 256)
        sw = None
        if i == 11:
            sw, c.family = {"NO_RAGGED": 1}, "gemm_kernel"
        add(c, "ragged", sw)

    # ---------------------------------------------------------------- fp32
    for i in range(8):   # chain3f: T >= 8192; the forward takes any d_out (D1 = d_in % 4 = 0), the backward any d_in
        T = g.randint(8192, 11000)
        if i < 3:
            d_in, d_out, edge = d.m8(128, 512) + 4 * (i % 2), 4 * g.randint(32, 128) + g.randint(1, 3), "c3f_dout_mod4"
        elif i < 6:
            d_in, d_out, edge = 4 * g.randint(32, 128) + g.randint(1, 3), d.m8(128, 512) + 4 * (i % 2), "c3f_din_mod4"
        else:
            d_in, d_out, edge = 4 * g.randint(33, 128), 4 * g.randint(33, 128), "c3f_aligned"
        c = Layer("", "f32", T, d_in, d_out, g.randint(1, 64), stratum="chain3f", family="chain3f_kernel", edges=(edge,))
        sw = None
        if i == 7:   # chain2f wants r >= 2
            sw, c.family, c.r = {"NO_CHAIN3F": 1}, "chain2f_kernel", max(c.r, 2)
        add(c, "chain3f", sw)
    for i in range(5):   # chain2f below 8192 (the short K / column split where >= 24 column tiles)
        T = g.choice([64, g.randint(65, 2000), g.randint(2000, 8191)])
        big = i % 2 == 0
        d_in = 4 * g.randint(200, 300) if big else 4 * g.randint(16, 128)
        d_out = 4 * g.randint(200, 300) if big else 4 * g.randint(16, 128)
        c = Layer("", "f32", T, d_in, d_out, g.randint(2, 64), stratum="chain2f", family="chain2f_kernel")
        add(c, "chain2f", {"F32_EXACT": 1} if i == 3 else None, h_null_ok=False)
    for i in range(5):   # the quad weight-gradient kernel (T >= 4096, >= 3 column groups each side) and its alternatives
        T = g.randint(4096, 8191)
        c = Layer("", "f32", T, 4 * g.randint(33, 160), 4 * g.randint(33, 160), g.randint(1, 64), stratum="tn_f32",
                  family="tn_partial_f32_quad_kernel")
        sw = None
        if i == 3:
            sw, c.family = {"NO_TN_F32Q": 1}, "tn_partial_dma_f32_wide_kernel"
        elif i == 4:
            sw, c.family = {"TN_NARROW": 1}, "tn_partial_dma_f32_kernel"
        add(c, "quad", sw)
    for i in range(3):   # tn_partial_dma_f32_wide: fewer than 3 column groups on one side
        c = Layer("", "f32", g.randint(64, 8191), 4 * g.randint(8, 32), 4 * g.randint(8, 200), g.randint(1, 64),
                  stratum="tn_f32", family="tn_partial_dma_f32_wide_kernel")
        add(c, "tnf32w")
    for i in range(3):   # gemm_x3: the fp32 dense accumulator, then the chain with beta = 1
        c = Layer("", "f32", g.randint(64, 9000), 4 * g.randint(16, 80), 4 * g.randint(16, 80), g.randint(1, 64),
                  acc="dense", stratum="gemm_x3", family="gemm_x3_kernel", y_rounds="twice", dx_rounds="twice")
        add(c, "gemm_x3", h_null_ok=False)

    # ---------------------------------------------------------------- generic kernels
    for i in range(12):
        dt = ("bf16", "f16", "f32")[i % 3]
        kind = i // 3
        T = g.randint(64, 8191)   # below chain3f's 8192
        d_in, d_out = d.m8(64, 520), d.m8(64, 520)
        r = d.even(4, 64)
        mis = 0
        if kind == 0:   # r odd, or 1, 2, 3
            r = g.choice([1, 2, 3, 2 * g.randint(2, 31) + 1]) if dt != "f32" else 1
            edge = "r_small_or_odd"
        elif kind == 1:
            T, edge = g.randint(1, 63), "T<64"
        elif kind == 2:   # r <= 64 at widths not a multiple of 8 (fp32: of 4)
            d_in, edge = d_in + g.randint(1, 7) if dt != "f32" else d_in + g.randint(1, 3), "ragged_r64"
        else:
            mis, edge = 1, "misaligned"
        c = Layer("", dt, T, d_in, d_out, r, misalign=mis, stratum="generic", family="chain_kernel", edges=(edge,))
        add(c, "generic")
    for c in out:
        if c.r > 64 and c.save_h is False and c.acc is not None:
            c.save_h = True
    return out


def _groups(d: _Draw) -> List[Group]:
    g = d.g
    out = []
    for i in range(12):
        dt = "f16" if i % 4 == 3 else "bf16"
        big = i % 3 == 0 and dt == "bf16"
        n = 4 if big else g.randint(2, 4)
        # big: four layers, the row-owner plan (tn_rows_plan: >= 160 slabs of >= 512 tokens over the group, <= 40 each)
        T = g.randint(16384, 20000) if big else g.randint(8193, 16000)
        layers = []
        for j in range(n):
            c = Layer(f"g{j}", dt, T, d.m8(256 if big else 128, 400), d.m8(256 if big else 128, 400), d.even(4, 64),
                      stratum="group")
            d.settings(c, h_null_ok=False)
            c.grad_beta = 0.0 if i % 2 == 0 else c.grad_beta
            if c.bias and c.r > 63:
                c.r = 62
            c.s = g.choice([1.0, 0.5, 2.0])
            layers.append(c)
        rows = dt == "bf16" and tn_rows_plan([T] * 2 * n, [v for c in layers for v in (c.d_in, c.d_out)])
        name = f"group{i}_{dt}_T{T}_" + "_".join(f"{c.d_in}x{c.d_out}r{c.r}" for c in layers)
        out.append(Group(name, layers, deferred=i % 2 == 1, rows=rows))
    return out


def _shared(d: _Draw) -> List[Shared]:
    g = d.g
    out = []
    for i in range(12):
        dt = "bf16" if i % 2 == 0 else "f16"
        T = g.randint(8193, 20000)
        d_in = d.m8(64, 512)
        sibs = [Sib(d.m8(8, 520), d.even(4, 64), g.random() < 0.5, g.choice([1.0, 0.5, 2.0])) for _ in range(g.randint(1, 4))]
        gb = g.choice([0.0, 0.5, 1.0])
        name = f"shared{i}_{dt}_T{T}_in{d_in}_" + "_".join(f"{sb.d_out}r{sb.r}" for sb in sibs)
        out.append(Shared(name, dt, T, d_in, sibs, gb))
    return out


def _gemms(d: _Draw) -> List[Gemm]:
    g = d.g
    out = []
    specs = []
    for i in range(30):   # random shapes 1 .. ~2300 in every dtype and transpose combination
        specs.append(("rand", ("bf16", "f16", "f32")[i % 3], g.randint(1, 2300), g.randint(1, 2300), g.randint(1, 2300), i))
    for i in range(6):    # >= 120 output tiles of 256 x 256 (gemm4)
        specs.append(("gemm4", ("bf16", "f16")[i % 2], g.randint(6 * 256 + 1, 7 * 256), d.m8(20 * 256 + 8, 24 * 256),
                      d.m8(512, 1024), i))
    for i in range(6):    # split-K: <= 128 tiles, tiles x splits >= 120, K >= 6144 -- with and without a workspace
        specs.append(("splitk", ("bf16", "f16")[i % 2], g.choice([1024, 1100]), g.choice([2048, 2056]), d.m8(6144, 6400), i))
    for i in range(6):    # bf16 gemm3s / gemm2_kernel (GEMM4 = 0)
        specs.append(("g3s" if i < 3 else "g2", "bf16", g.randint(1536, 2048), d.m8(1536, 2048), d.m8(512, 1024), i))
    for kind, dt, M, N, K, i in specs:
        if kind == "rand":
            ta, tb = bool(i & 1), bool(i & 2)
        else:
            ta, tb = False, bool(i & 1)
        # leading dimensions: the row length of each operand as stored, plus a gap (multiples of 8 keep the fast paths)
        rowa = M if ta else K
        rowb = K if tb else N
        pad = lambda: g.choice([0, 8, 16, g.randint(1, 7)]) if kind == "rand" else g.choice([0, 8, 24])   # noqa: E731
        lda, ldb, ldc = rowa + pad(), rowb + pad(), N + g.choice([8, 16]) if kind != "rand" else N + g.randint(1, 9)
        sw = {}
        use_ws = False
        if kind == "gemm4":
            fam = "gemm4_kernel" if dt == "bf16" else "gemm4_f16_kernel"
        elif kind == "splitk":
            use_ws = i < 4
            fam = ("gemm4_splitk_reduce_kernel" if dt == "bf16" else "gemm4_f16_splitk_reduce_kernel") if use_ws else (
                "gemm3s_kernel" if dt == "bf16" else "gemm_kernel")
        elif kind == "g3s":
            fam = "gemm3s_kernel"
        elif kind == "g2":
            fam, sw = "gemm2_kernel", {"GEMM4": 0, "GEMM3S": 0}
        else:
            fam = _gemm_family(dt, M, N, K, ta, tb, lda, ldb, ldc)
        alpha = g.choice([1.0, 0.5, -2.0])
        beta = g.choice([0.0, 0.5, 1.0])
        bias = g.random() < 0.5
        name = (f"gemm_{kind}_{dt}_{M}x{N}x{K}_{'T' if ta else 'N'}{'T' if tb else 'N'}_ld{lda}.{ldb}.{ldc}"
                f"_a{alpha:g}_b{beta:g}{'_bias' if bias else ''}{'_ws' if use_ws else ''}"
                + "".join(f"_{k}{v}" for k, v in sw.items()))
        out.append(Gemm(name, dt, M, N, K, ta, tb, lda, ldb, ldc, alpha, beta, bias, use_ws, sw, fam, d.n))
        d.n += 1
    return out


def _gemm_family(dt, M, N, K, ta, tb, lda, ldb, ldc):
    """sow_gemm_ex of api.hip for a random shape (no workspace): the kernel that writes C."""
    if ta:
        if dt == "f32":
            return "gemm_x3_kernel" if _x3_vec(M, N, K, ta, tb, lda, ldb, ldc) else "gemm_kernel"
        return "gemm_kernel"
    if dt == "f32":
        return "gemm_x3_kernel" if _x3_vec(M, N, K, ta, tb, lda, ldb, ldc) else "gemm_kernel"
    ok = N >= 64 and K >= 64 and K % 8 == 0 and N % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0
    if dt == "f16":
        return "gemm4_f16_kernel" if ok and cdiv(M, 256) * cdiv(N, 256) >= 120 else "gemm_kernel"
    t256, t128 = cdiv(M, 256) * cdiv(N, 256), cdiv(M, 128) * cdiv(N, 128)
    g2 = N >= 64 and K >= 32 and not (t256 < 160 and (t128 < 96 or K < 512))
    g2 = g2 and K % 8 == 0 and N % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0
    if not g2:
        return "gemm_kernel"
    if t256 >= 120 and K >= 64 and ok:
        return "gemm4_kernel"
    if t256 < 160:
        return "gemm3s_kernel"
    return "gemm3_kernel" if K >= 2048 else "gemm2_kernel"


def gemm2_ok(M, N, K):
    """The bf16 gate of pick_gemm (api.hip) for aligned bf16 operands with the defaults of the switches."""
    t256, t128 = cdiv(M, 256) * cdiv(N, 256), cdiv(M, 128) * cdiv(N, 128)
    return N >= 64 and K >= 32 and N % 8 == 0 and K % 8 == 0 and not (t256 < 160 and (t128 < 96 or K < 512))


def _x3_vec(M, N, K, ta, tb, lda, ldb, ldc):
    """launch_gemm_out's fp32 vector modes (16-byte aligned buffers): gemm_x3 needs all three and K >= 16."""
    def mode(ld, kcontig, rows):
        return (ld % 4 == 0 and K % 4 == 0) if kcontig else (ld % 4 == 0 and rows % 4 == 0)
    return mode(lda, not ta, M) and mode(ldb, tb, N) and ldc % 4 == 0 and N % 4 == 0 and K >= 16


# ---- the second stream: the kernel families that landed after the first sweep ------------------------------------------------
@dataclasses.dataclass
class Skinny:
    name: str
    dtype: str                  # "bf16" | "f16"
    kind: str                   # SK_KINDS: the accumulator of sow_forward_skinny
    T: int
    d_in: int
    d_out: int
    r: int
    bias: bool
    s: float
    f32: bool                   # fp32 factors (SOW_PARAM_F32 | SOW_ACC_NATIVE)
    seed: int


@dataclasses.dataclass
class SkinnyGroup:
    name: str
    dtype: str
    kind: str                   # the kind of the call's dense layers ("none": no layer has an accumulator)
    layers: List[Skinny]
    x_shared: bool              # every layer reads the first layer's x buffer (one T and d_in in the call)
    f32: bool


@dataclasses.dataclass
class Fused:
    name: str
    dtype: str
    T: int
    d_in: int
    d_out: int
    r: int
    r_acc: int
    bias: bool
    s: float
    save_h: bool
    group: bool                 # through sow_forward_group / sow_backward_group as a group of one
    deep: bool                  # SOW_FUSE_ACC_DEEP (r + r_acc > 256)
    seed: int


@dataclasses.dataclass
class AccSib:
    d_out: int
    r: int
    r_acc: int
    s: float


@dataclasses.dataclass
class SharedAcc:
    name: str
    dtype: str
    T: int
    d_in: int
    sibs: List[AccSib]
    grad_beta: float
    seed: int


SK_KINDS = ("dense", "e4m3", "mxfp4", "none")
SK_KS = (128, 256, 384, 512, 640, 768, 896, 1024)
SK_R_EDGES = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)   # around the x A tile counts (16 columns each)
SK_T_EDGES = (1, 15, 16, 17, 31, 32)                           # around the second row tile
SK_TAILS = ("kgroup", "partial", ">512", "full")
SK_COLS = ("lt", "8", "cn-8", "0")


def al256(n):
    return (n + 255) // 256 * 256


def r_pad(tot):
    return (tot + 63) // 64 * 64


def sk_cn(kind):
    """Columns per phase-A workgroup of the skinny forward: 128 for the code formats, else 64."""
    return 128 if kind in ("e4m3", "mxfp4") else 64


def sk_step(kind):
    """What d_in is a multiple of: whole MXFP4 blocks of 32, else one k-group of 8."""
    return 32 if kind == "mxfp4" else 8


def skinny_plan(d_in, d_out, kind):
    """skinny_fwd.hip skinny_plan: (slab count S, slab length KS, column ranges nc)."""
    nc = cdiv(d_out, sk_cn(kind)) if kind != "none" else 0
    want = cdiv(512, nc) if nc else 32
    ks = min(max(cdiv(cdiv(d_in, want), 128) * 128, 128), 1024)
    return cdiv(d_in, ks), ks, nc


def skinny_ws_bytes(T, d_in, d_out, kind):
    """api.hip skinny_ws: the answer of the three sow_forward_skinny*_workspace_bytes queries on an admitted shape."""
    S = skinny_plan(d_in, d_out, kind)[0]
    return 256 + (al256(S * T * d_out * 4) if kind != "none" else 0) + al256(S * T * 64 * 4)


def skinny_tail(d_in, d_out, kind):
    """Rows of the last K-slab."""
    S, ks, _ = skinny_plan(d_in, d_out, kind)
    return d_in - (S - 1) * ks


def skinny_tail_classes(d_in, d_out, kind):
    """SK_TAILS the last slab falls into: one k-group; otherwise no multiple of 128 (a partial round, idle waves); above 512
    (a fifth k-step refills the request ring); a whole slab."""
    tail, ks = skinny_tail(d_in, d_out, kind), skinny_plan(d_in, d_out, kind)[1]
    out = set()
    if tail == sk_step(kind):
        out.add("kgroup")
    elif tail % 128:
        out.add("partial")
    if tail > 512:
        out.add(">512")
    if tail == ks:
        out.add("full")
    return out


def skinny_col_class(d_out, kind):
    """SK_COLS of the last column range ("other": a residue the list does not name)."""
    cn = sk_cn(kind)
    if d_out < cn:
        return "lt"
    return {8: "8", cn - 8: "cn-8", 0: "0"}.get(d_out % cn, "other")


def fused_acc_shape_ok(r, r_acc, d_in, d_out, dtype):
    """chain_wide_acc.hip fused_acc_shape_ok: the admitted set of SOW_FUSE_ACC."""
    return (dtype in ("bf16", "f16") and 2 <= r <= 64 and r % 2 == 0 and r_acc >= 2 and r_acc % 2 == 0 and r_acc + r <= 256
            and d_in > 0 and d_out > 0 and d_in % 8 == 0 and d_out % 8 == 0)


def deep_acc_shape_ok(r, r_acc, d_in, d_out, dtype):
    """chain_deep_acc.hip deep_acc_shape_ok: the admitted set of SOW_FUSE_ACC_DEEP (DEEP_MAX_TOT = 960)."""
    return (dtype in ("bf16", "f16") and 2 <= r <= 64 and r % 2 == 0 and r_acc >= 2 and r_acc % 2 == 0 and r_acc <= 960
            and 256 < r_acc + r <= 960 and d_in > 0 and d_out > 0 and d_in % 8 == 0 and d_out % 8 == 0)


SHARED_ACC_MAX_LDS = 160 * 1024


def shared_acc_lds_bytes(r_tots):
    """chain_shared_acc.hip shared_acc_lds_bytes of the siblings' r + r_acc: 128 sum r_pad + max(128 max r_pad + 8192, 24576)
    (include/sow_amd.h); 0 outside 1 .. 4 siblings."""
    if not 1 <= len(r_tots) <= 4:
        return 0
    pads = [r_pad(t) for t in r_tots]
    return 128 * sum(pads) + max(128 * max(pads) + 8192, 24576)


def shared_acc_lds_ok(r_tots):
    b = shared_acc_lds_bytes(r_tots)
    return b != 0 and b <= SHARED_ACC_MAX_LDS


def sk_w_cap(kind, ks):
    """The largest d_in x d_out a drawn single-layer case takes at slab length ks: 1.5 x the smallest W that plans ks (an
    exhaustive search up to 9000 per side: 3.7 M elements per 128 rows of ks past the first for 64-column ranges, twice that
    for the code formats; 4104 x 8 and 8200 x 8 without an accumulator); at ks = 128 every width plans it, and 2 M (4 M) is taken."""
    if kind == "none":
        return {128: 1 << 20, 256: 1.5 * 4104 * 8, 384: 1.5 * 8200 * 8}[ks]
    return (sk_cn(kind) // 64) * (1.5 * 3.7e6 * (ks - 128) // 128 if ks > 128 else 2 << 20)


def _skinny_shape(g, kind, ks, tail, col, big_s):
    """(d_in, d_out) that plans slab length ks with the last slab in class `tail`, the last column range in class `col` and,
    for big_s, more than 16 slabs: d_out first (it fixes nc and want), then d_in inside the band of ks and under sk_w_cap."""
    cn, step, cap = sk_cn(kind), sk_step(kind), sk_w_cap(kind, ks)
    for _ in range(2000):
        if kind == "none" and ks > 128:
            d_out = 8
        else:
            if col == "lt":
                d_out = 8 * g.randint(1, cn // 8 - 1)
            else:
                # ranges: few where every width plans 128 rows, else as many as keep both sides under ~9000
                nc = g.randint(2, 16) if ks == 128 else g.randint(9000 // cn // 2, 9000 // cn)
                d_out = {"8": (nc - 1) * cn + 8, "cn-8": nc * cn - 8, "0": nc * cn}.get(col) or (nc - 1) * cn + 8 * g.randint(2, cn // 8 - 2)
        _, _, nc = skinny_plan(step, d_out, kind)
        want = cdiv(512, nc) if nc else 32
        lo = want * (ks - 128) + 1 if ks > 128 else step
        hi = min(want * ks if ks < 1024 else 1 << 30, int(cap // d_out), 8192 if ks == 128 else 1 << 30)
        cands = []
        for d_in in range(cdiv(lo, step) * step, hi + 1, step):
            S, k, _ = skinny_plan(d_in, d_out, kind)
            if k == ks and tail in skinny_tail_classes(d_in, d_out, kind) and (not big_s or S > 16):
                cands.append(d_in)
        if cands:
            # (the matrices of 12 M elements and more: the lower quarter of the band, for the float64 reference's sake)
            return g.choice(cands[:max(len(cands) // 4, 1)] if ks >= 512 else cands), d_out
    raise AssertionError(f"no skinny shape for {kind} KS {ks} tail {tail} col {col}")


def _sk_name(c: Skinny, tag):
    S, ks, _ = skinny_plan(c.d_in, c.d_out, c.kind)
    return (f"{tag}_{c.kind}_{c.dtype}_T{c.T}_{c.d_in}x{c.d_out}_r{c.r}_KS{ks}x{S}" + ("_bias" if c.bias else "")
            + ("_f32" if c.f32 else ""))


def _sk_settings(d: _Draw, c: Skinny):
    g = d.g
    c.bias = g.random() < 0.6
    c.s = g.choice([1.0, 0.5, 0.25, 1.0 / c.r])
    c.seed = d.n
    d.n += 1
    return c


# per dense kind: slab length, tail class, column class and "more than 16 slabs" of its 16 cases.  Every slab length is reached;
# one case at each length from 512 up (these are the 12 M to 58 M element matrices), the rest at 128, 256 and 384
_SK_DENSE = ([(128, t, c, b) for t, c, b in (("kgroup", "lt", False), ("partial", "lt", False), ("full", "8", False),
                                             ("kgroup", "cn-8", False), ("partial", "0", True))]
             + [(256, "full", "other", False), (256, "kgroup", "8", False), (256, "partial", "cn-8", False),
                (384, "full", "0", False), (384, "kgroup", "other", False), (384, "partial", "8", False),
                (512, "full", "cn-8", False), (640, ">512", "0", False), (768, ">512", "other", False), (896, ">512", "8", False),
                (1024, "partial", "cn-8", False)])
_SK_NONE = [(128, "kgroup", "8", False), (128, "partial", "cn-8", False), (128, "full", "0", False), (128, "partial", "lt", False),
            (256, "kgroup", "lt", True), (256, "partial", "lt", True), (384, "full", "lt", True), (384, "partial", "lt", True)]


def _skinny(d: _Draw) -> List[Skinny]:
    g = d.g
    specs = [(kind,) + sp for kind in SK_KINDS[:3] for sp in _SK_DENSE] + [("none",) + sp for sp in _SK_NONE]
    n = len(specs)
    # r uniform over 1 .. 64 and T over 1 .. 32, every edge value once; drawn again until 20 ranks are odd
    while True:
        rs, Ts = [g.randint(1, 64) for _ in range(n)], [g.randint(1, 32) for _ in range(n)]
        for v, i in zip(SK_R_EDGES, g.sample(range(n), len(SK_R_EDGES))):
            rs[i] = v
        for v, i in zip(SK_T_EDGES, g.sample(range(n), len(SK_T_EDGES))):
            Ts[i] = v
        if sum(r % 2 for r in rs) >= 20:
            break
    out = []
    for j, (kind, ks, tail, col, big_s) in enumerate(specs):
        d_in, d_out = _skinny_shape(g, kind, ks, tail, col, big_s)
        c = _sk_settings(d, Skinny("", "bf16" if j % 2 == 0 else "f16", kind, Ts[j], d_in, d_out, rs[j], True, 1.0, j % 3 == 0, 0))
        c.name = _sk_name(c, "sk")
        out.append(c)
    return out


def _skinny_groups(d: _Draw) -> List[SkinnyGroup]:
    g = d.g
    out = []
    calls = [(2, "dense"), (3, "e4m3"), (4, "mxfp4"), (7, "none"), (16, "dense"), (3, "e4m3"), (4, "mxfp4"), (2, "dense")]
    for i, (n, kind) in enumerate(calls):
        dt = "bf16" if i % 2 == 0 else "f16"
        x_shared, f32 = i in (2, 5), i in (0, 5)
        kinds = [kind] * n
        if kind != "none":   # one or two layers without an accumulator share the call
            for j in g.sample(range(n), 1 if n == 2 else g.randint(1, 2)):
                kinds[j] = "none"
        T0, din0 = g.randint(1, 32), 32 * g.randint(1, 32)
        layers = []
        for k in kinds:
            if x_shared:
                T, d_in = T0, din0
                d_out = d.m8(8, 1024)
            elif k == "none":   # d_in up to 12288: slabs of 256 and 384 rows next to the dense layers' 128
                T, d_in = g.randint(1, 32), g.choice([d.m8(8, 4096), d.m8(4104, 12288)])
                d_out = d.m8(8, min(1024, (1 << 20) // d_in))
            else:               # W <= 1 M elements
                T, d_out = g.randint(1, 32), d.m8(8, 1024)
                d_in = sk_step(k) * g.randint(1, min(4096, (1 << 20) // d_out) // sk_step(k))
            c = _sk_settings(d, Skinny("", dt, k, T, d_in, d_out, g.randint(1, 64), True, 1.0, f32, 0))
            if f32 and layers:   # (the fp32-factor runner of test_gpu_acc_native takes one scale per call)
                c.s = layers[0].s
            c.name = _sk_name(c, f"skg{i}.{len(layers)}")
            layers.append(c)
        name = f"skgroup{i}_{kind}_{dt}_n{n}" + ("_xshared" if x_shared else "") + ("_f32" if f32 else "")
        out.append(SkinnyGroup(name, dt, kind, layers, x_shared, f32))
    return out


def _fused_T(g, i):
    if i == 5:
        return g.randint(1000, 4200)
    if i % 2 == 0:
        return g.randint(1, 63)
    return 64 * g.randint(1, 6) + g.choice([-1, 0, 1])


def _split(g, tot, r=None):
    """(r, r_acc) of even parts with r <= 64 and r + r_acc = tot."""
    r = r or 2 * g.randint(1, min(64, tot - 2) // 2)
    return r, tot - r


def _fused(d: _Draw, deep: bool) -> List[Fused]:
    """16 layers of the SOW_FUSE_ACC set (deep: of SOW_FUSE_ACC_DEEP): the r_pad values in turn, r + r_acc drawn inside each;
    h_save = NULL for about an eighth (and for case 7), every fourth case as a group of one."""
    g = d.g
    out = []
    pads = list(range(320, 961, 64)) if deep else [64, 128, 192, 256]
    for i in range(16):
        pad = pads[i % len(pads)]
        tot = 2 * g.randint(max(pad - 62, 258 if deep else 4) // 2, pad // 2)
        r = None
        if deep:
            if i < 11 and pad in (320, 576, 832):   # the live columns [r_acc, r_acc + r) straddle the group boundary at pad - 64
                tot = pad - 64 + 2 * g.randint(1, 30)
                r = 2 * g.randint((tot - (pad - 64)) // 2 + 1, 32)
            elif pad in (384, 960) and i < 11:
                r = 64
        elif i < 3:                                 # (r + r_acc) % 64 of 0, 2 and 62
            tot = pad + (0, -62, -2)[i]
        r, r_acc = _split(g, tot, r)
        c = Fused("", "bf16" if i % 2 == 0 else "f16", _fused_T(g, i), d.m8(8, 600), d.m8(8, 600), r, r_acc, g.random() < 0.6,
                  1.0, i != 7 and g.random() >= 0.12, i % 4 == 3, deep, d.n)
        c.s = g.choice([1.0, 0.5, 1.0 / c.r, 2.0])
        d.n += 1
        assert (deep_acc_shape_ok if deep else fused_acc_shape_ok)(c.r, c.r_acc, c.d_in, c.d_out, c.dtype), c
        c.name = (f"{'deep' if deep else 'fused'}_{c.dtype}_T{c.T}_{c.d_in}x{c.d_out}_r{c.r}_acc{c.r_acc}" + ("_bias" if c.bias else "")
                  + ("" if c.save_h else "_noh") + ("_group" if c.group else ""))
        out.append(c)
    return out


def _shared_acc(d: _Draw) -> List[SharedAcc]:
    g = d.g
    out = []
    for i in range(8):
        dt = "f16" if i in (3, 6) else "bf16"
        if i == 0:     # 15 panels: 120 KiB of factors + 40 KiB of stage = exactly 160 KiB
            pads = [256, 256, 256, 192]
        else:
            while True:
                pads = [64 * g.randint(1, 4) for _ in range(4 if i == 1 else g.randint(1, 4))]
                if shared_acc_lds_ok(pads):
                    break
        sibs = []
        for pad in pads:
            r, r_acc = _split(g, 2 * g.randint(max(pad - 62, 4) // 2, pad // 2))
            sibs.append(AccSib(d.m8(24, 520), r, r_acc, g.choice([1.0, 0.5, 0.75])))
        T, d_in = g.randint(8193, 8800), d.m8(8, 520)
        name = f"sharedacc{i}_{dt}_T{T}_in{d_in}_" + "_".join(f"{sb.d_out}r{sb.r}a{sb.r_acc}" for sb in sibs)
        out.append(SharedAcc(name, dt, T, d_in, sibs, g.choice([0.0, 0.5, 1.0]), d.n))
        d.n += 1
    return out


def _ragged_dense(d: _Draw) -> List[Layer]:
    """Ragged widths with a dense accumulator: x W_acc by gemm_rag_kernel, then the ragged chain with beta = 1."""
    g = d.g
    out = []
    kinds = ("T<64", "T<256", "slab+1", "slab-1")
    for i in range(8):
        res = g.randint(1, 7)
        rag, other = 8 * g.randint(8, 70) + res, d.m8(64, 560)
        d_in, d_out = (rag, other) if i < 4 else (other, rag)
        kind = kinds[i % 4]
        c = Layer("", "bf16" if i % 2 == 0 else "f16", _wide_T(g, d_in, d_out, kind), d_in, d_out, d.even(66, 256), acc="dense",
                  stratum="ragged", family="gemm_rag_kernel", y_rounds="twice", dx_rounds="twice",
                  edges=(kind, f"rag_{'in' if i < 4 else 'out'}_{res}"))
        d.settings(c, h_null_ok=False)
        if i == 6:
            c.switches, c.family = {"NO_RAGGED_GEMM": 1}, "gemm_kernel"
        c.name = _name(c, "ragdense")
        out.append(c)
    return out


@dataclasses.dataclass
class Plan:
    layers: List[Layer]
    groups: List[Group]
    shared: List[Shared]
    gemms: List[Gemm]
    skinny: List[Skinny]
    skinny_groups: List[SkinnyGroup]
    fused: List[Fused]
    deep: List[Fused]
    shared_acc: List[SharedAcc]


N_FIRST_LAYERS = 103   # layers of the first stream; the second stream's dense ragged layers follow them in Plan.layers


def plan(seed: int = SEED) -> Plan:
    d = _Draw(seed)
    first = (_layers(d), _groups(d), _shared(d), _gemms(d))
    d2 = _Draw(seed + 1)     # a stream of its own: the four lists above stay what they were, case for case
    d2.n = 1000
    second = (_skinny(d2), _skinny_groups(d2), _fused(d2, False), _fused(d2, True), _shared_acc(d2))
    return Plan(first[0] + _ragged_dense(d2), *first[1:], *second)
