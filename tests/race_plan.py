"""The cases of tests/test_gpu_under_load.py (a plain module: importable without a GPU, no torch).

tests/graph_plan.py picks the smallest shape that selects a kernel family; at those shapes no LDS ring of the streaming
kernels is ever refilled (chain2 at 64 x 128: one X stage against 4 slots, three factor chunks against 6).  The cases here
are run while other work loads the chip (tests/under_load.py), so they take the smallest shapes at which the hand-ordered
waits of a kernel are actually needed:

Ring wrap.  For every LDS ring a claimed kernel cycles through, the trip count of the case is at least 3 x the slot count,
and the last trip is partial where the kernel admits one (a width 8 past a multiple of the stage, a token count 1 past a
multiple of the block).  RINGS holds, per case, rows (source file, constant, slots, unit, trips); tests/test_race_plan_cpu.py
reads the constant out of the source (names and integers only) and asserts slots and trips >= 3 * slots, so a ring that is
deepened later turns that test red.  A case lists the rings it wraps and only those; every ring below is wrapped by at least one.

The rings (the kernels that order LDS by hand: every file that includes lds_dma.hpp and issues dma16):
  chain2.hip:87-90        C2_DEPTH = 4 X stages [32 tok][64 k] per token group, C2_NSLOT = 6 factor chunks of 64 rows, fed
                          C2_AHEAD = 5 ahead (4 in a row-aligned launch); trips: ceil(D1 / 64) stages -- D1 = d_in forward,
                          d_out backward -- and ceil(d_in / 64) + ceil(d_out / 64) chunks per block; the park tiles of phase 2
                          rotate through 2 (fp32) or 3 (16-bit) buffers inside the X ring (chain2.hip:539, 635), once per slice
  chain2_shared.hip:31-34 CS_DEPTH = 4, CS_NSLOT = 6, CS_AHEAD = 5: the same rings, the X stream shared by the siblings
  chain2f.hip:57-59       C3_DEPTH = 3 X stages [32 tok][64 k] fp32, C3_NSLOT = 2 factor chunks
  chain3f.hip:35          C4_XDEPTH = 3 X stages; the factor planes double-buffered (chain3f.hip:38, C4_RING0 = 2 * C4_FSLOT)
  skinny_tn.hip:218       TN_DEPTH = 4 stages of 16 tokens per wave, 4 waves (tn_partial_dma_kernel, TN_NARROW)
  skinny_tn.hip:396       TNW_DEPTH = 3 stages of 16 tokens per wave, TNW_WAVES = 8 (tn_partial_dma_wide_kernel)
  skinny_tn.hip:603       TNR_DEPTH = 4 stages of 16 or 32 tokens per workgroup (tn_partial_rows_kernel)
  skinny_tn.hip:827       TNF_DEPTH = 4 stages of 8 tokens per wave, 4 waves (tn_partial_dma_f32_kernel)
  skinny_tn.hip:1025      TNFW_DEPTH = 4 stages of 8 tokens per wave, TNFW_WAVES = 6 (tn_partial_dma_f32_wide_kernel)
  skinny_tn_f32q.hip:28   TNQ_DEPTH = 3 stages of 32 tokens per workgroup (tn_partial_f32_quad_kernel)
  gemm2.hip:35, gemm3.hip:20, gemm2h.hip:32   G2_NSLOT = G3_NSLOT = GH_NSLOT = 4 stages of 32 k
  gemm3s.hip:24           GS_NSLOT = 4 stages of 64 k
  gemm4.hip:43-44         two K-tile buffers of four half-tiles (G4_LDS = 2 * G4_BUF), K-tiles of 64 k (+ the extension tile);
                          gemm4h's projection pass: three buffers (gemm4_body.hpp:151, tl % 3), one trip per K-tile
The token-slab rings of the weight-gradient kernels turn once per 16 (8, 32) tokens of a slab; the slab length is the C
plan's (tn_pick_slabs, mirrored below), never longer than about T / 16 + 64 at these widths, so they wrap
3 x only in the cases with many tokens or few slabs; the per-case rows say where.

Every other kernel keeps ONE LDS image per workgroup between __syncthreads() (compiler-visible LDS accesses, which hipcc
orders itself): chain.hip:95, chain_wide.hip:70, chain_wide_acc.hip:44, chain_deep_acc.hip:54, chain_shared_acc.hip:77,
skinny_fwd.hip:149, skinny_tn_wide.hip:26-28, gemm.hip:164, gemm_x3.hip:126, gemm_rag.hip:102, qr_blocked.hip:40, and the
reductions of the optimizer, grad_stats, colsum, the pack kernels, the TT helpers, QR, accumulate and dequantise.  They have
no ring to wrap and take their graph_plan case as it is.

More than one block per workgroup.  A persistent grid carries LDS state from one block to the next.  MULTI holds, per case,
(source file, the constant of the resident grid, blocks): the CPU test reads the constant and asserts
2 * grid < blocks < 3 * grid, so that workgroups 0 .. blocks - 2 * grid - 1 run three blocks and the others two.
  chain2.hip:879    launch_chain2_group: grid = min(blocks, C2_RESIDENT = 512) unless NO_PERSIST; blocks = ceil(T / 64) per
                    layer; workgroup g runs blocks g, g + 512, ... (chain2.hip:753)
  chain2_shared.hip:615   the same with CS_RESIDENT = 512 over ceil(T / 64) blocks
  skinny_tn.hip           launch_tn_group: grid = min(blocks, 256); blocks = sum over the layers of a grouped launch of
                    (pairs of 64-column groups) x slabs.  One layer never exceeds 256 (tn_pick_slabs keeps it in one round), a
                    group of three 776-wide layers does.
The other grids are one workgroup per tile or slab: the GEMM kernels use gridDim only for the XCD remap (there is no resident
tile loop), tn_partial_rows_kernel's plan (tn_rows_plan, skinny_tn.hip) admits 160 .. 256 blocks against a grid of 256.
T past 2 * 512 * 64 tokens is what the chain2 case costs; at the ring-wrap widths (776 x 776) its buffers (360 MB) and its
float64 reference (8e10 multiply-adds) would break both caps below, so the chain2 case takes the widest shape the caps leave
(712 x 72: the forward X ring wraps, 14 chunks against 6 slots), the shared one 72 -> 72 + 136, and the ring-wrap cases the
smallest T.

Caps (tests/test_race_plan_cpu.py): the float64 reference of a case stays under the cost of the most expensive case of
fuzz_plan.plan(); the buffers of a case (case_bytes) under 256 MiB.

`claims`, EXEMPT and kernel_names() are those of graph_plan.py: every __global__ of the sources is claimed by a case here.
"""
from __future__ import annotations

import collections
import os
import re
from typing import Dict, List, Tuple

import fuzz_plan as FP
import graph_plan as GP

L = FP.Layer
Case = GP.Case
cdiv = FP.cdiv
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sow_amd", "csrc")

# (source file, constant, slots, unit of one trip, trips of this case): a case lists the rings it wraps, and only those
Ring = collections.namedtuple("Ring", "file name slots unit trips")
# (source file, constant of the resident grid, blocks of the launch)
Multi = collections.namedtuple("Multi", "file name blocks")

EXEMPT: Dict[str, str] = {}
MAX_BYTES = 256 << 20
RINGS: Dict[str, Tuple[Ring, ...]] = {}
MULTI: Dict[str, Multi] = {}


# constants the tables name that are literals in the sources: name -> (file, pattern with one integer group)
LITERALS = {
    "G4_PA_RING": ("gemm4_body.hpp", r"char\* buf = smem \+ \(tl % (\d+)\) \* G4_PA_BUF;"),
    "TNW_RESIDENT": ("skinny_tn.hip", r"\(sw_on\(SW_NO_PERSIST\) \|\| total < (\d+)\) \? total : \1;\s+// one resident workgroup per CU"),
}


def constant(file: str, name: str, csrc: str = None) -> int:
    """The integer a `constexpr int NAME = ...;` or `#define NAME ...` of the source gives: a literal, another such name, or
    `<integer> * <name>` (gemm4.hip's G4_LDS = 2 * G4_BUF stands for its two K-tile buffers: the factor is returned).  A name of
    LITERALS stands for a literal of the one source line its pattern matches."""
    if name in LITERALS:
        file, pat = LITERALS[name]
    with open(os.path.join(csrc or CSRC, file)) as f:
        text = f.read()
    if name in LITERALS:
        m = re.search(pat, text)
        assert m, f"{file}: the line that holds {name} changed"
        return int(m.group(1))
    for _ in range(4):
        m = (re.search(r"constexpr int (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % re.escape(name), text)
             or re.search(r"^\s*#\s*define\s+%s\s+(\S+)\s*$" % re.escape(name), text, re.M))
        assert m, f"{file}: no constant {name}"
        v = m.group(1).strip()
        if re.fullmatch(r"\d+", v):
            return int(v)
        k = re.fullmatch(r"(\d+) \* \w+", v)
        if k:
            return int(k.group(1))
        assert re.fullmatch(r"\w+", v), f"{file}: {name} = {v}"
        name = v
    raise AssertionError(f"{file}: {name} does not resolve")


# ---- the slab plan of the weight-gradient kernels (skinny_tn.hip: tn_pick_slabs, api.hip: plan_ws) ---------------------------
def tn_slabs(T, d_in, d_out, dtype, narrow=False):
    """(slab count, slab length) of one layer's weight-gradient launch."""
    cg_in, cg_out = cdiv(d_in, 64), cdiv(d_out, 64)
    bt = 32 if dtype == "f32" else 64
    max_ns = max(cdiv(T, 512), 1)
    if dtype == "f32" and narrow:
        ns = max(min(512 // (cg_in + cg_out), max_ns), 1)
        if ns > 8 and (ns & ~7) * 10 >= ns * 9:
            ns &= ~7
    else:
        cg2 = max(cdiv(cg_in, 2) + cdiv(cg_out, 2), 1)
        ns = (256 // cg2) & ~7
        if ns < 8 or dtype == "f32":
            ns = 256 // cg2
        if dtype == "f32" and not narrow and T >= 4096 and cg_in >= 3 and cg_out >= 3:      # the quad kernel
            ns = 256 // (cdiv(cg_in, 4) + cdiv(cg_out, 4))
            if ns >= 8:
                ns &= ~7
        ns = max(min(ns, max_ns), 1)
    ln = max(cdiv(cdiv(T, ns), bt) * bt, bt)
    return max(cdiv(T, ln), 1), ln


def tn_wave_trips(T, d_in, d_out, dtype, tokens, waves, narrow=False):
    """Trips of a per-wave token ring in the first slab: stages of `tokens` tokens dealt round-robin to `waves` waves."""
    ns, ln = tn_slabs(T, d_in, d_out, dtype, narrow)
    return cdiv(cdiv(min(ln, T), tokens), waves)


def tn_wide_blocks(T, d_in, d_out, dtype):
    ns, _ = tn_slabs(T, d_in, d_out, dtype)
    return (cdiv(cdiv(d_in, 64), 2) + cdiv(cdiv(d_out, 64), 2)) * ns


# ---- ring rows by family -------------------------------------------------------------------------------------------------------
def _chain_rows(file, depth, nslot, d_in, d_out):
    return (Ring(file, depth, 0, "64 k of the streamed operand (forward d_in, backward d_out)", min(cdiv(d_in, 64), cdiv(d_out, 64))),
            Ring(file, nslot, 0, "64-row factor chunk", cdiv(d_in, 64) + cdiv(d_out, 64)))


def _slots(rows):
    return tuple(r._replace(slots=constant(r.file, r.name)) for r in rows)


def _add(case, rows=(), multi=None):
    if rows:
        RINGS[case.id] = _slots(rows)
    if multi:
        MULTI[case.id] = multi
    return case


W, TW = 776, 8193 + 64            # 13 stages of 64 k, the last of 8; 130 token blocks, the last of 1 token
WA, TA = 1376, 9217 + 64          # 21.5 lines per row (the row-aligned launch); slabs of 1216 tokens
TM = 2 * 512 * 64 + 4097          # 1089 token blocks on 512 resident workgroups: 65 run three, 447 two


def _tn_row(lay, name, tokens, waves, narrow=False):
    return Ring("skinny_tn.hip", name, 0, f"{tokens} tokens of a slab, per wave ({waves} waves)",
                tn_wave_trips(lay.T, lay.d_in, lay.d_out, lay.dtype, tokens, waves, narrow))


def _chain2_case(tag, lay, claims, extra=(), **kw):
    c = GP._layer(tag, lay, claims, **kw)
    return _add(c, _chain_rows("chain2.hip", "C2_DEPTH", "C2_NSLOT", lay.d_in, lay.d_out) + tuple(extra))


def _layers():
    out = []
    # chain2, fp32 park tiles (bias, grad_beta): 13 stages both ways, 26 chunks
    lay = L("", "bf16", TW, W, W, 50, s=0.5, grad_beta=1.0)
    out.append(_chain2_case("chain2", lay, ("chain2_kernel", "tn_partial_dma_wide_kernel", "tn_reduce_kernel")))
    # 16-bit park tiles, pair flush (no bias, beta = 0), f16
    lay = L("", "f16", TW, W, W, 50, bias=False)
    out.append(_chain2_case("chain2", lay, ("chain2_f16_kernel", "tn_partial_dma_wide_kernel")))
    # the cache-policy and hand-off switches of test_gpu_stream_policy.py keep their switch
    out.append(_chain2_case("chain2", L("", "bf16", TW, W, W, 50, bias=False, switches={"NT_LOAD": 1, "NO_NT_STORE": 1}),
                            ("chain2_kernel",)))
    out.append(_chain2_case("chain2", L("", "f16", TW, W, W, 50, s=0.5, switches={"NO_H_ROWS": 1}), ("chain2_f16_kernel",)))
    # the row-aligned launch (1376 columns: the loaders run 4 ahead, chunk c - 1 stays alive through step c); slabs of 1216
    # tokens wrap the wide weight-gradient ring (9.5 stages per wave), under TN_NARROW the narrow one (19)
    lay = L("", "bf16", TA, WA, WA, 50, bias=False)
    out.append(_chain2_case("chain2al", lay, ("chain2_kernel", "tn_partial_dma_wide_kernel"), (_tn_row(lay, "TNW_DEPTH", 16, 8),)))
    lay = L("", "bf16", TA, WA, WA, 50, bias=False, s=2.0, switches={"TN_NARROW": 1})
    out.append(_chain2_case("chain2al", lay, ("chain2_kernel", "tn_partial_dma_kernel"), (_tn_row(lay, "TN_DEPTH", 16, 4, narrow=True),)))
    out.append(_chain2_case("chain2al", L("", "f16", TA, WA, WA, 50, bias=False, switches={"NO_ROW_ALIGN": 1}),
                            ("chain2_f16_kernel",)))
    # more blocks than resident workgroups, at the widest shape the caps leave at this T: the forward X ring wraps (712 = 11 x 64
    # + 8: 12 stages), the chunk ring is refilled (12 + 2 chunks against 6 slots); slabs of 2240 tokens wrap the wide
    # weight-gradient ring too
    lay = L("", "bf16", TM, 712, 72, 50, s=0.5)
    c = GP._layer("multi", lay, ("chain2_kernel", "tn_partial_dma_wide_kernel"))
    out.append(_add(c, (Ring("chain2.hip", "C2_DEPTH", 0, "64 k of x (the forward launch)", cdiv(712, 64)), _tn_row(lay, "TNW_DEPTH", 16, 8)),
                    Multi("chain2.hip", "C2_RESIDENT", cdiv(TM, 64))))
    # dense accumulator: gemm4h bounds N (two column tiles), not K, and each direction is admitted on its own.  584 x 456: the
    # forward (N = 456, K = 584 = 9 x 64 + 8) makes 10 K-tiles in the three-buffer projection pass and 11 in the main loop; its
    # data gradient (N = 584: three tiles) leaves gemm4h for the fused streaming product.  456 x 456: gemm4h both ways, f16.
    # gemm2h (K = 392: 13 stages of 32)
    out.append(_add(GP._layer("gemm4h", L("", "bf16", 60 * 256 + 1, 584, 456, 16, acc="dense", s=0.5), ("gemm4_kernel",)),
                    (Ring("gemm4.hip", "G4_LDS", 0, "K-tile of 64 k (+ the extension tile)", cdiv(584, 64) + 1),
                     Ring("gemm4.hip", "G4_PA_RING", 0, "K-tile of 64 k of the projection pass", cdiv(584, 64)))))
    out.append(_add(GP._layer("gemm4h", L("", "f16", 60 * 256 + 1, 456, 456, 16, acc="dense", bias=False), ("gemm4_f16_kernel",)),
                    (Ring("gemm4.hip", "G4_LDS", 0, "K-tile of 64 k (+ the extension tile)", cdiv(456, 64) + 1),)))
    out.append(_add(GP._layer("gemm2h", L("", "bf16", 80 * 256 + 1, 392, 392, 16, acc="dense", switches={"NO_GEMM4H": 1}),
                              ("gemm2h_kernel",)), (Ring("gemm2h.hip", "GH_NSLOT", 0, "stage of 32 k", cdiv(392, 32)),)))
    # fp32: chain3f + the quad weight-gradient kernel (slabs of 512 tokens: 16 stages of 32), chain2f + the wide / narrow ones
    lay = L("", "f32", TW, W, W, 16, s=0.5)
    ns, ln = tn_slabs(lay.T, W, W, "f32")
    out.append(_add(GP._layer("chain3f", lay, ("chain3f_kernel", "chain3f_planes_kernel", "tn_partial_f32_quad_kernel")),
                    _chain_rows("chain3f.hip", "C4_XDEPTH", "C4_RING0", W, W)
                    + (Ring("skinny_tn_f32q.hip", "TNQ_DEPTH", 0, "32 tokens of a slab", cdiv(ln, 32)),)))
    lay = L("", "f32", 1000, W, W, 16)
    out.append(_add(GP._layer("chain2f", lay, ("chain2f_kernel", "tn_partial_dma_f32_wide_kernel")),
                    _chain_rows("chain2f.hip", "C3_DEPTH", "C3_NSLOT", W, W)))
    # the wide fp32 weight-gradient kernel past 4096 tokens: an operand with fewer than 3 column groups keeps the layer off the
    # quad kernel (tn_shape_kernel); 32 slabs of 576 tokens: 72 stages of 8 tokens over 6 waves
    lay = L("", "f32", 276 * 64 + 1, W, 128, 16, s=0.5)
    out.append(_add(GP._layer("tnf32w", lay, ("chain3f_kernel", "tn_partial_dma_f32_wide_kernel")), (_tn_row(lay, "TNFW_DEPTH", 8, 6),)))
    lay = L("", "f32", 1000, W, W, 16, s=0.5, switches={"TN_NARROW": 1})
    out.append(_add(GP._layer("chain2f", lay, ("chain2f_kernel", "tn_partial_dma_f32_kernel")),
                    _chain_rows("chain2f.hip", "C3_DEPTH", "C3_NSLOT", W, W) + (_tn_row(lay, "TNF_DEPTH", 8, 4, narrow=True),)))
    return out


LAYERS = _layers()


def _groups():
    # three 776-wide layers, weight gradients deferred: one grouped launch of the wide kernel with 3 x 210 blocks on 256
    # resident workgroups (118 run three blocks, 138 two), then every reduction in one sow_reduce_batch launch
    widths = [(W, W, 16, True, 0.5), (W, W, 8, False, 1.0), (W, W, 50, True, 2.0)]
    c = GP._group("deferred", "bf16", TW, widths, True, False, ("tn_reduce_batch_kernel", "tn_partial_dma_wide_kernel", "chain2_kernel"))
    blocks = sum(tn_wide_blocks(TW, d_in, d_out, "bf16") for d_in, d_out, *_ in widths)
    return [_add(c, _chain_rows("chain2.hip", "C2_DEPTH", "C2_NSLOT", W, W), Multi("skinny_tn.hip", "TNW_RESIDENT", blocks))]


GROUPS = _groups()


def _shared(tag, T, d_in, sibs):
    cid = f"shared_{tag}_bf16_T{T}_in{d_in}_" + "_".join(f"{o}r{r}" for o, r, *_ in sibs)
    return Case(cid, "shared", dict(dtype="bf16", T=T, d_in=d_in, sibs=sibs, grad_beta=1.0), ("chain2_shared_kernel",),
                (T, d_in) + tuple(v for o, r, *_ in sibs for v in (o, r)), sum(14.0 * T * (d_in + o) * 64 for o, *_ in sibs))


SHARED = [
    _add(_shared("wrap", TW, W, [(W, 16, False, 0.5), (W, 8, True, 1.0)]),
         (Ring("chain2_shared.hip", "CS_DEPTH", 0, "64 k of x (forward) / of a sibling's dY (backward)", cdiv(W, 64)),
          Ring("chain2_shared.hip", "CS_NSLOT", 0, "64-row factor chunk", 2 * (cdiv(W, 64) + cdiv(W, 64))))),
    _add(_shared("multi", TM, 72, [(72, 16, False, 0.5), (136, 8, True, 1.0)]), (),
         Multi("chain2_shared.hip", "CS_RESIDENT", cdiv(TM, 64))),
]

KG = 776                     # 13 stages of 64 k (25 of 32), the last of 8
GEMMS = [
    _add(GP._gemm("bf16", 5120, 1536, 584, ("gemm4_kernel",)), (Ring("gemm4.hip", "G4_LDS", 0, "K-tile of 64 k", cdiv(584, 64)),)),
    _add(GP._gemm("bf16", 1536, 1024, KG, ("gemm3s_kernel",), beta=1.0), (Ring("gemm3s.hip", "GS_NSLOT", 0, "stage of 64 k", cdiv(KG, 64)),)),
    _add(GP._gemm("bf16", 1536, 1024, KG, ("gemm2_kernel",), switches={"GEMM3S": 0}),
         (Ring("gemm2.hip", "G2_NSLOT", 0, "stage of 32 k", cdiv(KG, 32)),)),
    _add(GP._gemm("bf16", 1536, 1024, KG, ("gemm3_kernel",), switches={"GEMM3S": 0, "GEMM3": 1}),
         (Ring("gemm3.hip", "G3_NSLOT", 0, "stage of 32 k", cdiv(KG, 32)),)),
]

# ---- the graph_plan cases that stay as they are ----------------------------------------------------------------------------------
# replaced above by a ring-wrap or multi-block case of the same kernels
REPLACED = {
    "layer_chain2_bf16_T8193_64x128_r16", "layer_chain2_f16_T8193_128x64_r16", "layer_chain2_bf16_T8193_72x136_r8_TN_NARROW1",
    "layer_gemm4h_bf16_T15361_264x264_r16_dense", "layer_gemm4h_f16_T15361_264x264_r16_dense",
    "layer_gemm2h_bf16_T20481_264x264_r16_dense_NO_GEMM4H1", "layer_chain3f_f32_T8193_256x264_r16",
    "layer_chain2f_f32_T1000_128x128_r16", "layer_chain2f_f32_T1000_128x128_r16_TN_NARROW1",
    "group_deferred_bf16_T8193_64x128r16_64x72r8_128x64r4", "shared_bf16_T8193_in64_64r16_128r8",
    "gemm_bf16_5120x1536x512", "gemm_bf16_1536x1024x512_b1", "gemm_bf16_1536x1024x512_GEMM3S0",
    "gemm_bf16_1536x1024x512_GEMM3S0_GEMM31",
}
AS_IS = [c for c in GP.CASES if c.id not in REPLACED]
assert len(AS_IS) == len(GP.CASES) - len(REPLACED), sorted(REPLACED - {c.id for c in GP.CASES})


def _as_is_rows():
    """The graph_plan shapes that already wrap a ring: the split-K products (K = 6144: 24 K-tiles per split, gemm3s at
    K = 2048) and the row-owner group (slabs of 544 tokens)."""
    by = {c.id: c for c in AS_IS}
    g4 = Ring("gemm4.hip", "G4_LDS", 0, "K-tile of 64 k of one split", cdiv(cdiv(6144, 64), 4))
    for cid in ("gemm_bf16_1024x2048x6144_ws", "gemm_f16_1024x2048x6144_ws_b1"):
        _add(by[cid], (g4,))
    _add(by["layer_splitk_bf16_T1024_6144x2048_r16_dense"],
         (g4._replace(trips=cdiv(cdiv(6144, 64) + 1, 4)), Ring("gemm3s.hip", "GS_NSLOT", 0, "stage of 64 k", cdiv(2048, 64) + 1)))
    rows = next(c for c in AS_IS if c.kind == "group" and c.p["rows"])
    T = rows.p["layers"][0].T
    ns = min(256 // (2 * len(rows.p["layers"])), T // 512)
    ln = cdiv(cdiv(T, ns), 32) * 32
    _add(rows, (Ring("skinny_tn.hip", "TNR_DEPTH", 0, "32 tokens of a slab", cdiv(ln, 32)),))


_as_is_rows()

CASES: List[Case] = LAYERS + GROUPS + SHARED + GEMMS + AS_IS

def claimed() -> set:
    return {k for c in CASES for k in c.claims}


def switches(case) -> dict:
    if case.kind == "layer":
        return dict(case.p["layer"].switches)
    return dict(case.p.get("switches", {}))


def case_bytes(c) -> int:
    """Bytes of the operands, outputs and the saved projections of a case (the workspaces of these shapes are a few per cent of
    that; 10 % is added for them and the guards)."""
    es = {"bf16": 2, "f16": 2, "f32": 4}

    def layer(m):
        acc = m.d_in * m.d_out if m.acc == "dense" else (m.d_in + m.d_out) * m.r_acc
        return es[m.dtype] * (m.T * (2 * m.d_in + 2 * m.d_out + 2 * max(m.r, 64)) + 2 * (m.d_in + m.d_out) * m.r + acc)

    if c.kind == "layer":
        n = layer(c.p["layer"])
    elif c.kind == "group":
        n = sum(layer(m) for m in c.p["layers"])
    elif c.kind == "shared":
        p = c.p
        n = 2 * (2 * p["T"] * p["d_in"] + sum(p["T"] * (2 * o + 128) for o, *_ in p["sibs"]))
    elif c.kind == "gemm":
        p = c.p
        n = es[p["dtype"]] * (p["M"] * p["K"] + p["K"] * p["N"] + p["M"] * p["N"]) + (4 * 4 * p["M"] * p["N"] if p["use_ws"] else 0)
    else:
        return 64 << 20          # the optimizer, TT, QR, skinny and fused cases of graph_plan.py: a few MB each
    return int(1.1 * n)
