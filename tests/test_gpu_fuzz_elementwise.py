"""-m gpu: the seeded random sweep of tests/fuzz_plan.py through the element-wise checks of tests/test_gpu_elementwise.py.

Every dispatch family of sow_forward / sow_backward_ex, the grouped and shared-input entry points and sow_gemm_ex runs on
drawn shapes with NaN-neighboured inputs, sentinel guards and three runs (poisoned, zeroed, poisoned) that must be
bit-identical.  The third run is traced (torch.profiler):
* the kernel family the plan targets has to appear -- a case that falls back to another kernel fails;
* the rounding class of y and of dX is read off the trace (a fused single-accumulator path rounds once; an accumulator
  product followed by the chain with beta = 1 rounds twice) and has to agree with the plan's;
* test_zz_fuzz_coverage (last) asserts that every family of fuzz_plan.FAMILIES was reached by >= 3 cases and prints the
  counts and the worst err / limit of the cases that ran each family.
"""
import ctypes

import pytest
import torch

import fuzz_plan as FP
import test_gpu_elementwise as E
import test_gpu_shared_input as S
from numerics import check_bound, check_gaps, fp32_floor, gemm_epilogue, gemm_f32_bound, to64
from sow_amd import _lib

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
                          "gemm4_f16_splitk_reduce_kernel")
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


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_zz_fuzz_coverage():
    """Every family of fuzz_plan.FAMILIES reached by >= 3 drawn cases; prints the counts and the worst err / limit of the
    cases that ran each family (run with -s)."""
    planned = len(PLAN.layers) + len(PLAN.groups) + len(PLAN.shared) + len(PLAN.gemms)
    if len(RAN) < planned:
        pytest.skip(f"the coverage check runs after the whole sweep ({len(RAN)} of {planned} cases ran)")
    for fam in FP.FAMILIES:
        w, case = WORST.get(fam, (float("nan"), ""))
        print(f"family {fam:58s} cases {len(SEEN.get(fam, ())):4d}  worst err/limit {w:.3f}  ({case})")
    short = {f: len(SEEN.get(f, ())) for f in FP.FAMILIES if len(SEEN.get(f, ())) < 3}
    assert not short, f"families reached by fewer than 3 cases: {short}"
