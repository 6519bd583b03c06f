"""-m gpu: the seeded random sweep of tests/fuzz_plan.py through the element-wise checks of tests/test_gpu_elementwise.py.

Every dispatch family of sow_forward / sow_backward_ex, the grouped and shared-input entry points and sow_gemm_ex runs on
drawn shapes with NaN-neighboured inputs, sentinel guards and three runs (poisoned, zeroed, poisoned) that must be
bit-identical.  The third run is traced (torch.profiler):
* the kernel family the plan targets has to appear -- a case that falls back to another kernel fails;
* the rounding class of y and of dX is read off the trace (a fused single-accumulator path rounds once; an accumulator
  product followed by the chain with beta = 1 rounds twice) and has to agree with the plan's;
* the second stream of the plan runs each family through that family's own runner and comparator: the skinny forward
  (test_gpu_skinny, test_gpu_fp8_acc, test_gpu_fp4_acc, the fp32-factor runner of test_gpu_acc_native) on operands cleared of
  rounding ties (skinny_sweep.py), the fused accumulator passes (test_gpu_fused_acc, test_gpu_deep_acc), the shared-input data
  gradient of low-rank siblings (test_gpu_shared_fused_acc); the dense ragged layers are cases of test_fuzz_layer;
* test_zz_fuzz_coverage (last) asserts that every family of fuzz_plan.FAMILIES was reached by >= 3 cases and prints the
  counts and the worst err / limit of the cases that ran each family.
"""
import ctypes

import pytest
import torch

import fp4_acc_ref as R4
import fused_acc_numerics as FA
import fuzz_plan as FP
import shared_fused_acc_numerics as SN
import skinny_sweep as SW
import test_gpu_acc_native as AN
import test_gpu_deep_acc as DE
import test_gpu_elementwise as E
import test_gpu_fp4_acc as F4
import test_gpu_fp8_acc as F8
import test_gpu_fused_acc as FU
import test_gpu_shared_fused_acc as SA
import test_gpu_shared_input as S
import test_gpu_skinny as SK
from numerics import check_bound, check_gaps, check_h_save, fp32_floor, gemm_epilogue, gemm_f32_bound, to64
from sow_amd import _lib, acc_quant

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PLAN = FP.plan()

CHAINS = ("chain2_kernel", "chain2_f16_kernel", "chain_kernel", "chain3f_kernel", "chain2f_kernel", "chain_wide_kernel",
          "chain2_shared_kernel")
GEMMS = ("gemm_kernel", "gemm_x3_kernel", "gemm2_kernel", "gemm2h_kernel", "gemm3_kernel", "gemm3s_kernel", "gemm4_kernel",
         "gemm4_f16_kernel")
KNOWN = CHAINS + GEMMS + ("h_reduce_kernel", "tn_partial_dma_kernel", "tn_partial_dma_wide_kernel", "tn_partial_rows_kernel",
                          "tn_partial_kernel", "tnw_partial_kernel", "tn_partial_f32_quad_kernel", "tn_partial_dma_f32_kernel",
                          "tn_partial_dma_f32_wide_kernel", "colsum_kernel", "gemm4_splitk_reduce_kernel",
                          "gemm4_f16_splitk_reduce_kernel", "gemm_rag_kernel")
SEEN = {}        # family label -> set of case names
WORST = {}       # family label -> (worst err / limit, case)
RAN = set()      # cases that reached their checks


def _is(name, kernel):
    # demangled ("sow::chain_kernel<...>") or mangled ("_ZN3sow12chain_kernel...") names of exactly this kernel
    return f"sow::{kernel}" in name or f"{len(kernel)}{kernel}" in name


def _has(seq, kernel):
    return any(_is(n, kernel) for n in seq)


def _main(seq):
    """The chain / GEMM launches of a trace, in order: ("chain" | "gemm", kernel)."""
    out = []
    for n in seq:
        for k in CHAINS:
            if _is(n, k):
                out.append(("chain", k))
        for k in GEMMS:
            if _is(n, k):
                out.append(("gemm", k))
    return out


def _rounds(seq, acc):
    """Rounding class of the output of one direction, from its trace: without an accumulator one kernel writes y (or dX)
    from operands the test sees ("once"); with one, "once" only where the accumulator product and the low-rank term share
    one fp32 accumulator -- gemm2h, gemm4h (one gemm4 launch, nothing else but weight-gradient kernels after it), or the
    H-only chain pass followed by the GEMM with the rank extension; an accumulator product (GEMM or chain) followed by
    another y-writing launch with beta = 1 is "twice"."""
    if acc is None:
        return "once"
    m = _main(seq)
    if acc == "dense" and m:
        if m[0][1] == "gemm2h_kernel":
            return "once"
        if m[0][1] in ("gemm4_kernel", "gemm4_f16_kernel") and (len(m) == 1 or m[1][0] not in ("chain", "gemm")):
            return "once"
        if m[0][0] == "chain" and len(m) > 1 and m[1][0] == "gemm":
            return "once"
    return "twice"


def _labels(seq, layer=None):
    """The coverage labels of a trace (fuzz_plan.FAMILIES)."""
    out = set()
    for k in KNOWN:
        if not _has(seq, k):
            continue
        if k == "chain_wide_kernel":
            rag = layer is not None and (layer.d_in % 8 or layer.d_out % 8)
            out.add("chain_wide_kernel[ragged]" if rag else "chain_wide_kernel[aligned]")
        elif k == "gemm4_kernel":
            if _has(seq, "gemm4_splitk_reduce_kernel"):
                out.add("gemm4_kernel[splitk]")
            else:
                m = _main(seq)
                fused = layer is not None and layer.acc == "dense" and layer.r <= 64 and m and m[0][1] == "gemm4_kernel"
                out.add("gemm4_kernel[h]" if fused else "gemm4_kernel[plain]")
        else:
            out.add(k)
    for fam in FP.FAMILIES:   # alternatives: "a|b"
        if "|" in fam and any(a in out for a in fam.split("|")):
            out.add(fam)
    return out


def _note(name, labels, worst):
    RAN.add(name)
    for lab in labels:
        SEEN.setdefault(lab, set()).add(name)
        if worst is not None and worst > WORST.get(lab, (-1.0, ""))[0]:
            WORST[lab] = (worst, name)


def _case_worst(name):
    ws = [w for (c, _), (w, _) in E.WORST.items() if c == name]
    return max(ws) if ws else None


def _to_case(c: FP.Layer, y_rounds, dx_rounds, name=None):
    return E.Case(name or c.name, DT[c.dtype], c.T, c.d_in, c.d_out, c.r, acc=c.acc, r_acc=c.r_acc, bias=c.bias, s=c.s,
                  grad_beta=c.grad_beta, misalign=c.misalign, switches=dict(c.switches), y_rounds=y_rounds,
                  save_h=c.save_h, seed=c.seed, dx_rounds=dx_rounds)


# ---------------------------------------------------------------------------------------------------------------- layers
@pytest.mark.parametrize("c", PLAN.layers, ids=lambda c: c.name)
def test_fuzz_layer(c):
    case = _to_case(c, c.y_rounds, c.dx_rounds)
    d = E._inputs(case)
    trace = {}
    out = E._run_single(case, d, trace)
    seq = trace["fwd"] + trace.get("bwd", [])
    assert _has(seq, c.family), f"{c.name}: targets {c.family}, the trace holds {sorted(set(seq))}"
    y_r = _rounds(trace["fwd"], c.acc)
    dx_r = _rounds(trace.get("bwd", []), c.acc)
    assert y_r == c.y_rounds, f"{c.name}: y rounds {y_r} by the trace {trace['fwd']}, the plan says {c.y_rounds}"
    if c.save_h:
        assert dx_r == c.dx_rounds, f"{c.name}: dX rounds {dx_r} by the trace {trace['bwd']}, the plan says {c.dx_rounds}"
    labels = _labels(seq, c)
    try:
        E._check(case, d, out)
    finally:
        _note(c.name, labels, _case_worst(c.name))


# ---------------------------------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("gp", PLAN.groups, ids=lambda g: g.name)
def test_fuzz_group(gp):
    layers = [_to_case(c, "once", "once", name=f"{gp.name}.{c.name}") for c in gp.layers]
    data = [E._inputs(c) for c in layers]
    outs, seq = run_group(gp, layers, data)
    labels = _labels(seq)
    try:
        for i, c in enumerate(layers):
            E._check(c, data[i], outs[i])
    finally:
        ws = [w for w in (_case_worst(c.name) for c in layers) if w is not None]
        _note(gp.name, labels, max(ws) if ws else None)


def run_group(gp, layers, data):
    """The grouped forward and backward of `layers` (test_gpu_elementwise.Case) on the operands `data` (one dict per layer,
    as E._inputs gives): three runs (poisoned, zeroed, poisoned) that must be bit-identical, guards intact, the row-owner
    plan as the trace shows it.  Returns (outputs of the first run per layer, on the CPU; kernel names of the third)."""
    lib = _lib.load()
    dtype = DT[gp.layers[0].dtype]
    dt = E._dt(dtype)
    ar = E.Arena(dtype)
    arr = (_lib.LayerArgs * len(layers))()
    bufs = []
    for i, (c, d) in enumerate(zip(layers, data)):
        b = dict(x=ar.input(d["x"]), A=ar.input(d["A"]), B=ar.input(d["B"]), bias=ar.input(d["bias"]), dy=ar.input(d["dy"]),
                 y=ar.output((c.T, c.d_out)), h=ar.output((c.T, 64), misalign=0), dx=ar.output((c.T, c.d_in)),
                 dA=ar.output((c.d_in, c.r), d.get("dA0"), misalign=0), dB=ar.output((c.r, c.d_out), d.get("dB0"), misalign=0),
                 dbias=ar.output((c.d_out,), d.get("dbias0"), misalign=0) if c.bias else None)
        b["ws"] = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, _lib.ACC_NONE, dt))
        bufs.append(b)
        arr[i] = _lib.LayerArgs(x=E._ptr(b["x"]), A=E._ptr(b["A"]), B=E._ptr(b["B"]), acc_down=None, acc_up=None,
                                bias=E._ptr(b["bias"]), y=E._ptr(b["y"]), h_save=E._ptr(b["h"]), dy=E._ptr(b["dy"]),
                                dx=E._ptr(b["dx"]), dA=E._ptr(b["dA"]), dB=E._ptr(b["dB"]), dbias=E._ptr(b["dbias"]), T=c.T,
                                d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=0, acc_kind=_lib.ACC_NONE, scale=c.s,
                                grad_beta=c.grad_beta, workspace=E._ptr(b["ws"]), workspace_bytes=b["ws"].numel())
    n = len(layers)
    phases = (_lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS) if gp.deferred else (_lib.BWD_DATA | _lib.BWD_WEIGHTS)
    slabs = (ctypes.c_int * (2 * n))()
    rows = lib.sow_backward_group_plan(arr, n, dt, phases, slabs)
    assert rows in (0, 1), rows
    descs = starts = None
    total = 0
    if gp.deferred:
        size = lib.sow_reduce_desc_bytes()
        raw = ctypes.create_string_buffer(size * n)
        blocks = (ctypes.c_int * n)()
        _lib.check(lib.sow_backward_group_reduce_desc(arr, n, dt, phases, raw, blocks), "sow_backward_group_reduce_desc")
        descs = torch.frombuffer(bytearray(raw.raw), dtype=torch.uint8).to(DEV)
        st = []
        for k in range(n):
            st.append(total)
            total += blocks[k]
        starts = torch.tensor(st, dtype=torch.int32, device=DEV)

    def step():
        _lib.check(lib.sow_forward_group(arr, n, dt, E._stream()), "sow_forward_group")
        _lib.check(lib.sow_backward_group(arr, n, dt, phases, E._stream()), "sow_backward_group")
        if gp.deferred:
            _lib.check(lib.sow_reduce_batch(E._ptr(descs), E._ptr(starts), n, total, dt, E._stream()), "sow_reduce_batch")

    keys = ("y", "h", "dx", "dA", "dB", "dbias")
    runs = []
    seq = []
    for byte in (0xFF, 0x00, 0xFF):
        ar.fill(byte)
        if len(runs) == 2:
            seq = E._kernel_seq(step)
        else:
            step()
        ar.check_guards(f"{gp.name} run {len(runs)}")
        runs.append([{k: (None if b[k] is None else b[k].clone()) for k in keys} for b in bufs])
    assert bool(rows) == _has(seq, "tn_partial_rows_kernel"), \
        f"{gp.name}: sow_backward_group_plan says {rows}, the trace holds {sorted(set(seq))}"
    for i, c in enumerate(layers):
        for k in keys:
            if runs[0][i][k] is not None:
                assert torch.equal(E._bits(runs[0][i][k]), E._bits(runs[1][i][k])), f"{c.name}: {k} differs on zeroed memory"
                assert torch.equal(E._bits(runs[0][i][k]), E._bits(runs[2][i][k])), f"{c.name}: {k} differs on a repeat"
    return [{k: (None if v is None else v.cpu()) for k, v in runs[0][i].items()} for i in range(n)], seq


# ---------------------------------------------------------------------------------------------------------------- shared
@pytest.mark.parametrize("sp", PLAN.shared, ids=lambda s: s.name)
def test_fuzz_shared(sp):
    dtype = DT[sp.dtype]
    st = shared_set(sp)
    x, per, dx0 = S._data(st, seed=FP.SEED % 1000)
    b, runs, seq = run_shared(st, x, per, dx0)
    labels = _labels(seq)
    names = []
    try:
        for j, (sb, p) in enumerate(zip(st.sibs, b.inp)):
            c = E.Case(f"{sp.name}.s{j}", dtype, st.T, st.d_in, sb.d_out, sb.r, bias=sb.bias, s=sb.s)
            names.append(c.name)
            d = dict(x=b.x.cpu(), A=p["A"].cpu(), B=p["B"].cpu(), bias=None if p["bias"] is None else p["bias"].cpu(),
                     dy=p["dy"].cpu())
            E._check(c, d, {k: (None if v is None else v.cpu()) for k, v in runs[0][0][j].items()})
        ref, bnd = S._dx_reference(st, b, dx0)
        if dtype == torch.float16:   # dh rounded to f16 hides a subnormal floor as well (test_gpu_elementwise._sub_term)
            aa = sum((to64(p["A"]) ** 2).sum(1) for p in b.inp)
            bnd = bnd + E._sub_term(aa[None, :].expand(st.T, -1), dtype)
        stx = check_bound(runs[0][1].cpu(), ref, bnd, name=f"{sp.name}: dX")
        E.WORST[(f"{sp.name}.s0", "dx_sum")] = (stx["worst"], None)
    finally:
        ws = [w for w in (_case_worst(nm) for nm in names) if w is not None]
        _note(sp.name, labels, max(ws) if ws else None)


def shared_set(sp):
    return S.Set(sp.name, DT[sp.dtype], sp.T, sp.d_in, [S.Sib(sb.d_out, sb.r, sb.bias, sb.s) for sb in sp.sibs],
                 grad_beta=sp.grad_beta)


def run_shared(st, x, per, dx0):
    """sow_forward_shared + sow_backward_shared of the sibling set `st` on the operands x, per (one dict of A, B, bias, dy
    per sibling) and dx0 (as test_gpu_shared_input._data gives): three bit-identical runs, guards intact, the shared
    kernel in the trace.  Returns (the bound buffers, the runs: ([per-sibling outputs], dX), kernel names of the third)."""
    lib = _lib.load()
    dtype = st.dtype
    b = S.Bound(st, x, per, dx0)
    n, dt = len(st.sibs), S._dt(dtype)
    sh = b.sets["shared"]

    def step():
        _lib.check(lib.sow_forward_shared(b.args("shared"), n, dt, E._stream()), "sow_forward_shared")
        _lib.check(lib.sow_backward_shared(b.args("shared"), n, dt, _lib.BWD_DATA | _lib.BWD_WEIGHTS, E._stream()),
                   "sow_backward_shared")

    keys = ("y", "h", "dA", "dB", "dbias")
    runs = []
    seq = []
    for byte in (0xFF, 0x00, 0xFF):
        b.ar.fill(byte)
        if len(runs) == 2:
            seq = E._kernel_seq(step)
        else:
            step()
        b.ar.check_guards(f"{st.name} run {len(runs)}")
        runs.append(([{k: (None if o[k] is None else o[k].clone()) for k in keys} for o in sh], sh[0]["dx"].clone()))
    for i in (1, 2):
        assert torch.equal(E._bits(runs[0][1]), E._bits(runs[i][1])), f"{st.name}: dX differs between runs"
        for j in range(n):
            for k in keys:
                if runs[0][0][j][k] is not None:
                    assert torch.equal(E._bits(runs[0][0][j][k]), E._bits(runs[i][0][j][k])), f"{st.name}: {k} of sibling {j}"
    assert _has(seq, "chain2_shared_kernel"), f"{st.name}: the trace holds {sorted(set(seq))}"
    return b, runs, seq


# ---------------------------------------------------------------------------------------------------------------- gemm
def _strided_input(vals, ld, dtype):
    """[rows, cols] values in a [rows, ld] buffer whose gaps and guards hold NaN."""
    rows, cols = vals.shape
    buf = torch.full((rows * ld + 2 * E.GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[E.GUARD:E.GUARD + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(vals.to(DEV, dtype))
    return buf, view


@pytest.mark.parametrize("gm", PLAN.gemms, ids=lambda g: g.name)
def test_fuzz_gemm(gm):
    dtype = DT[gm.dtype]
    g = torch.Generator().manual_seed(5000 + gm.seed)
    M, N, K = gm.M, gm.N, gm.K
    a = torch.randn(M, K, generator=g).to(dtype)               # op(A)
    bm = (torch.randn(K, N, generator=g) * 0.05).to(dtype)     # op(B)
    bias = (torch.randn(N, generator=g) * 0.1).to(dtype) if gm.bias else None
    c0 = torch.randn(M, N, generator=g).to(dtype) if gm.beta else None
    out, seq = run_gemm(gm, a, bm, bias, c0)
    a64, b64 = to64(a), to64(bm)
    prod = a64 @ b64
    ref = gm.alpha * prod + (to64(bias) if bias is not None else 0) + (gm.beta * to64(c0) if c0 is not None else 0)
    sq = gm.alpha ** 2 * ((a64 * a64) @ (b64 * b64))
    epi = gemm_epilogue(prod, gm.alpha, gm.beta, c0 if gm.beta else None, bias)
    try:
        if dtype == torch.float32:
            st = check_bound(out, ref, gemm_f32_bound(ref, sq, gm.alpha * prod, K, epi), name=gm.name)
            E.WORST[(gm.name, "C")] = (st["worst"], None)
        else:
            st = E._rounded(out, ref, dtype, fp32_floor(sq, K) + epi, gm.name)
            E.WORST[(gm.name, "C")] = (st["worst"], st["inexact"])
    finally:
        _note(gm.name, _labels(seq), _case_worst(gm.name))


def run_gemm(gm, a, bm, bias, c0):
    """sow_gemm_ex of the case `gm` on the operands op(A) = a [M, K], op(B) = bm [K, N], bias [N] or None and C0 [M, N] or
    None (tensors of the case's dtype): strided NaN-gapped inputs, a sentinel-gapped C, three bit-identical runs, the
    targeted kernel in the trace.  Returns (C of the first run on the CPU, kernel names of the third)."""
    lib = _lib.load()
    dtype = DT[gm.dtype]
    dt = E._dt(dtype)
    M, N, K = gm.M, gm.N, gm.K
    _, A = _strided_input(a.t() if gm.trans_a else a, gm.lda, dtype)
    _, B = _strided_input(bm.t() if gm.trans_b else bm, gm.ldb, dtype)
    ar = E.Arena(dtype)
    Bi = ar.input(bias)
    cbuf = torch.full((M * gm.ldc + 2 * E.GUARD,), E.SENTINEL, dtype=dtype, device=DEV)
    C = cbuf[E.GUARD:E.GUARD + M * gm.ldc].view(M, gm.ldc)[:, :N]
    live = torch.zeros(cbuf.numel(), dtype=torch.bool, device=DEV)
    live[E.GUARD:E.GUARD + M * gm.ldc].view(M, gm.ldc)[:, :N] = True
    with _lib.switch(**gm.switches):
        nws = lib.sow_gemm_workspace_bytes(M, N, K, int(gm.trans_a), dt) if gm.use_ws else 0
        assert (nws > 0) == gm.use_ws, f"{gm.name}: workspace query {nws}"
        ws = ar.workspace(nws)

        def call():
            _lib.check(lib.sow_gemm_ex(E._ptr(A), gm.lda, int(gm.trans_a), E._ptr(B), gm.ldb, int(gm.trans_b), E._ptr(C), gm.ldc,
                                       E._ptr(Bi), M, N, K, gm.alpha, gm.beta, dt, E._ptr(ws), nws, E._stream()), "sow_gemm_ex")

        runs = []
        seq = []
        for byte in (0xFF, 0x00, 0xFF):
            ar.fill(byte)
            if gm.beta:
                C.copy_(c0.to(DEV))
            else:
                E._bits(C).fill_(-1 if byte == 0xFF else 0)
            if len(runs) == 2:
                seq = E._kernel_seq(call)
            else:
                call()
            torch.cuda.synchronize()
            check_gaps(cbuf.cpu(), live.cpu(), E.SENTINEL, name=f"{gm.name} run {len(runs)}")
            runs.append(C.clone())
    assert torch.equal(E._bits(runs[0]), E._bits(runs[1])) and torch.equal(E._bits(runs[0]), E._bits(runs[2])), \
        f"{gm.name}: runs differ"
    assert _has(seq, gm.family), f"{gm.name}: targets {gm.family}, the trace holds {sorted(set(seq))}"
    return runs[0].cpu(), seq


# ---------------------------------------------------------------------------------------------------------------- skinny
def _quant4(W):
    """test_gpu_fp4_acc._quant; matrices past 1 M elements through the package's quantiser on the GPU, which
    test_gpu_fp4_acc.test_quantiser_* tie to the reference bit for bit (as test_gpu_fp8_acc._quant does)."""
    if W.numel() <= 1 << 20:
        return F4._quant(W)
    q, e = acc_quant.quantize_tensor(W.to(DEV), "mxfp4")
    codes, scales = q.cpu(), e.cpu()
    return codes, scales, R4.dequantize(codes, scales, W.dtype)


# per accumulator kind: (runner, comparator, the prefix under which the comparator files its worst ratio, quantiser, label)
SKINNY = {"dense": (SK._run, SK._check, "", None, "skinny_a_kernel[plain]"),
          "none": (SK._run, SK._check, "", None, "skinny_a_kernel[plain]"),
          "e4m3": (F8._run, F8._check, "fp8_", F8._quant, "skinny_a_kernel[e4m3]"),
          "mxfp4": (F4._run, F4._check, "fp4_", _quant4, "skinny_a_kernel[mxfp4]")}


def _ours(seq):
    """The library's kernels of a trace (the rest: torch's fills and copies of the buffer protocol)."""
    return [k for k in seq if "sow::" in k or "3sow" in k]


def _skinny_trace(seq, name):
    """One launch of each skinny kernel and nothing else of the library: nothing else writes y."""
    ours = _ours(seq)
    a, b = sum(_is(k, "skinny_a_kernel") for k in ours), sum(_is(k, "skinny_b_kernel") for k in ours)
    assert a == 1 and b == 1 and len(ours) == 2, f"{name}: the trace holds {ours}"


def _skinny_query(c, code):
    """The workspace query of the case's kind under the dtype code `code`, asserted equal to the plan's mirror."""
    lib = _lib.load()
    if c.kind == "e4m3":
        got = lib.sow_forward_skinny_fp8_workspace_bytes(c.T, c.d_in, c.d_out, c.r, code)
    elif c.kind == "mxfp4":
        got = lib.sow_forward_skinny_fp4_workspace_bytes(c.T, c.d_in, c.d_out, c.r, code)
    else:
        got = lib.sow_forward_skinny_workspace_bytes(c.T, c.d_in, c.d_out, c.r, AN.KINDS[c.kind], code)
    want = FP.skinny_ws_bytes(c.T, c.d_in, c.d_out, c.kind)
    assert got == want, f"{c.name}: the workspace query says {got}, fuzz_plan.skinny_ws_bytes {want}"


def _skinny_runs(run, dtype, ds, x_shared, name):
    """Three runs of one sow_forward_skinny call through the family's runner (poisoned, zeroed: bit-identical, guards intact;
    poisoned again on fresh buffers, traced: bit-identical to the first).  Returns (the y of the first run, the trace)."""
    ys = run(dtype, ds, x_shared=x_shared, runs=(0xFF, 0x00), what=name)
    third = []
    seq = E._kernel_seq(lambda: third.extend(run(dtype, ds, x_shared=x_shared, runs=(0xFF,), what=name + " (traced)")))
    for i, (a, b) in enumerate(zip(ys, third)):
        assert torch.equal(E._bits(a), E._bits(b)), f"{name}: y of layer {i} differs on the traced run"
    _skinny_trace(seq, name)
    return ys, seq


def _native_layer(c, d):
    """The case's operands as test_gpu_acc_native._skinny reads them: fp32 masters that round to the factors."""
    q_down = d.get("q") if c.kind in ("e4m3", "mxfp4") else d["W"]
    return dict(x=d["x"], A=SW.fp32_master(d["A"]), B=SW.fp32_master(d["B"]), bias=None if d["bias"] is None else SW.fp32_master(d["bias"]),
                q_down=AN._dev(q_down), q_up=AN._dev(d.get("e")), kind=AN.KINDS[c.kind])


def _native_runs(cs, ds, s, x_shared, name):
    """The call on fp32 factors (SOW_PARAM_F32 | SOW_ACC_NATIVE), traced; returns its y per layer on the CPU."""
    cd = SW.DT[cs[0].dtype]
    for c in cs:
        _skinny_query(c, AN.CODE[cd] | AN.PF | AN.NATIVE)
    layers = [_native_layer(c, d) for c, d in zip(cs, ds)]
    got = []
    seq = E._kernel_seq(lambda: got.extend(AN._skinny(cd, layers, True, s=s, x_shared=x_shared)))
    _skinny_trace(seq, name + " (fp32 factors)")
    return [y.cpu() for y in got]


@pytest.mark.parametrize("c", PLAN.skinny, ids=lambda c: c.name)
def test_fuzz_skinny(c):
    dtype = SW.DT[c.dtype]
    run, check, prefix, quantise, label = SKINNY[c.kind]
    d, moved = SW.operands(c, quantise)
    print(f"{c.name}: {moved} of {d['A'].numel()} elements of A moved by one ulp")
    _skinny_query(c, E._dt(dtype))
    (y,), seq = _skinny_runs(run, dtype, [d], False, c.name)
    labels = {label, "skinny_b_kernel"}
    if c.f32:   # fp32 factors: the bits of the call on the pre-rounded ones
        (y32,) = _native_runs([c], [d], c.s, False, c.name)
        assert torch.equal(E._bits(y32), E._bits(y)), f"{c.name}: fp32 factors differ from the pre-rounded call"
        labels.add("skinny_a_kernel[fp32-factors]")
    try:
        check(c.name, dtype, d, y)
    finally:
        _note(c.name, labels, SK.WORST.get(prefix + c.name))


@pytest.mark.parametrize("gp", PLAN.skinny_groups, ids=lambda g: g.name)
def test_fuzz_skinny_group(gp):
    dtype = SW.DT[gp.dtype]
    run, check, prefix, quantise, label = SKINNY[gp.kind]
    x0 = None
    ds = []
    for c in gp.layers:
        d, _ = SW.operands(c, quantise, x=x0)
        x0 = d["x"] if gp.x_shared else None
        _skinny_query(c, E._dt(dtype))
        ds.append(d)
    grouped, seq = _skinny_runs(run, dtype, ds, gp.x_shared, gp.name)
    labels = {label, "skinny_b_kernel"}
    calls = [("grouped", grouped)]
    if gp.f32:
        calls.append(("grouped on fp32 factors", _native_runs(gp.layers, ds, gp.layers[0].s, gp.x_shared, gp.name)))
        labels.add("skinny_a_kernel[fp32-factors]")
    try:
        for i, (c, d) in enumerate(zip(gp.layers, ds)):
            (single,) = run(dtype, [d], runs=(0xFF,), what=c.name)
            for what, ys in calls:
                assert torch.equal(E._bits(ys[i]), E._bits(single)), f"{gp.name}: y of layer {i} of the {what} call differs from its call alone"
            check(c.name, dtype, d, single)
    finally:
        ws = [SK.WORST[prefix + c.name] for c in gp.layers if prefix + c.name in SK.WORST]
        _note(gp.name, labels, max(ws) if ws else None)


# ---------------------------------------------------------------------------------------------------------------- fused, deep
def _fuzz_fused(c, flags, trace_check, label):
    case = FA.case(c.name, DT[c.dtype], c.T, c.d_in, c.d_out, c.r, c.r_acc, s=c.s, bias=c.bias, seed=c.seed)
    d = E._inputs(case)
    trace = {}
    out = FU._run(case, d, flags=flags, trace=trace, save_h=c.save_h, group=c.group)
    # h_save = NULL: the forward only -- its trace is held to the rule of both directions
    trace_check(dict(trace, bwd=trace.get("bwd", trace["fwd"])), c.name)
    worst = {}
    try:
        worst = FA.check(case, d, out)
        if out.get("dh") is not None:   # dh, which the weight kernels read (test_fused_layer_elementwise)
            dy, B = to64(d["dy"]), to64(d["B"])
            st = check_h_save(to64(out["dh"]), c.s * (dy @ B.t()), c.r, case.dtype,
                              acc=fp32_floor(c.s * c.s * ((dy * dy) @ (B * B).t()), c.d_out), name=f"{c.name}: dh")
            worst["dh"] = st["worst"]
        for k in ("y", "h", "dx", "dA", "dB", "dbias"):
            assert out.get(k) is None or not torch.isnan(out[k].float()).any(), f"{c.name}: poison left in {k}"
    finally:
        _note(c.name, {label}, max(worst.values()) if worst else None)


@pytest.mark.parametrize("c", PLAN.fused, ids=lambda c: c.name)
def test_fuzz_fused(c):
    _fuzz_fused(c, FU.FUSE, FU._fused_trace, "chain_wide_acc_kernel")


@pytest.mark.parametrize("c", PLAN.deep, ids=lambda c: c.name)
def test_fuzz_deep(c):
    _fuzz_fused(c, DE.DEEP, DE._deep_trace, "chain_deep_acc_kernel")


# ---------------------------------------------------------------------------------------------------------------- shared_acc
@pytest.mark.parametrize("sp", PLAN.shared_acc, ids=lambda s: s.name)
def test_fuzz_shared_acc(sp):
    """test_gpu_shared_fused_acc's buffers and calls: the flagged grouped forward and backward, then sow_backward_shared on the
    grouped call's h -- three times (poisoned, zeroed, poisoned)."""
    lib = _lib.load()
    st = SN.Set(sp.name, DT[sp.dtype], sp.T, sp.d_in, [SN.Sib(sb.d_out, sb.r, sb.r_acc, s=sb.s) for sb in sp.sibs],
                grad_beta=sp.grad_beta, seed=sp.seed)
    assert FP.shared_acc_lds_ok([sb.r + sb.r_acc for sb in sp.sibs])
    d = SN.inputs(st)
    b = SA.Bound(st, d)
    n, flag = len(st.sibs), SA._flag(st)
    hs = b.sets["group"]
    both = SA.DATA | SA.WEIGHTS

    def shared():
        rc = lib.sow_backward_shared(b.args("shared", h_from=hs), n, flag, both, E._stream())
        assert rc == 0, f"{sp.name}: sow_backward_shared returned {rc}"

    runs, seq = [], []
    for byte in (0xFF, 0x00, 0xFF):
        b.ar.fill(byte)
        _lib.check(lib.sow_forward_group(b.args("group"), n, flag, E._stream()), "sow_forward_group")
        _lib.check(lib.sow_backward_group(b.args("group"), n, flag, both, E._stream()), "sow_backward_group")
        if len(runs) == 2:
            seq = E._kernel_seq(shared)
        else:
            shared()
        b.ar.check_guards(f"{sp.name} run {len(runs)}")
        for i, (og, os_) in enumerate(zip(b.sets["group"], b.sets["shared"])):
            for k in ("dA", "dB", "dbias"):
                if og[k] is not None:
                    assert torch.equal(E._bits(og[k]), E._bits(os_[k])), \
                        f"{sp.name}: {k} of sibling {i} differs from the grouped path (dh is not bit-identical)"
        runs.append(b.sets["shared"][0]["dx"].clone())
    assert torch.equal(E._bits(runs[0]), E._bits(runs[1])) and torch.equal(E._bits(runs[0]), E._bits(runs[2])), \
        f"{sp.name}: dX differs between runs"
    assert _has(seq, "chain_shared_acc_kernel") and not _has(seq, "chain_wide_acc_kernel"), f"{sp.name}: the trace holds {_ours(seq)}"
    worst = None
    try:
        worst = SN.check_dx(st, d, runs[0].cpu())["worst"]
    finally:
        _note(sp.name, {"chain_shared_acc_kernel"}, worst)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_zz_fuzz_coverage():
    """Every family of fuzz_plan.FAMILIES reached by >= 3 drawn cases; prints the counts and the worst err / limit of the
    cases that ran each family (run with -s)."""
    planned = sum(len(v) for v in (PLAN.layers, PLAN.groups, PLAN.shared, PLAN.gemms, PLAN.skinny, PLAN.skinny_groups, PLAN.fused,
                                   PLAN.deep, PLAN.shared_acc))
    if len(RAN) < planned:
        pytest.skip(f"the coverage check runs after the whole sweep ({len(RAN)} of {planned} cases ran)")
    for fam in FP.FAMILIES:
        w, case = WORST.get(fam, (float("nan"), ""))
        print(f"family {fam:58s} cases {len(SEEN.get(fam, ())):4d}  worst err/limit {w:.3f}  ({case})")
    short = {f: len(SEEN.get(f, ())) for f in FP.FAMILIES if len(SEEN.get(f, ())) < 3}
    assert not short, f"families reached by fewer than 3 cases: {short}"
