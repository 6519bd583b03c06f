"""-m gpu: every dispatch path of sow_forward / sow_backward / the grouped entry points / sow_gemm, checked element by
element against float64 references (tests/numerics.py), with guard bands and poisoned memory.

The C ABI is called through `_lib` with raw pointers, so that the test owns every buffer:
* every input is a view into a larger buffer whose neighbours hold NaN (a read past the view shows up as NaN in an output,
  even where the kernel would multiply it by zero); one case per kernel family offsets its views by one element, which
  breaks 16-byte alignment and drives the generic fallback;
* every output has a leading and a trailing guard holding a sentinel that must survive the call;
* outputs and the workspace are filled with 0xFF bytes (NaN in both dtypes) before the call; a second run on zeroed
  memory and a third on poisoned memory again must give bit-identical results (the kernels have no float atomics);
* the stages are checked from the kernel's own visible intermediates: h_save (contract of DESIGN section 3:
  RNE(s x A) in columns < r, 0 up to column 62, 1.0 in column 63 when r <= 63), y from h_save, dB and dbias from h_save
  and dY (check_rounded); dA and dX, whose dh the test cannot see, against check_bound; fp32 everywhere with check_bound.

Rounding classification of y (`y_rounds` of a case):
* "once": chain2 / chain_short / generic chain (no accumulator), gemm4h, gemm2h, chain_short + split-K gemm2 (the dense
  product and the low-rank term in one accumulator), the r > 64 composition without an accumulator (one GEMM writes y);
* "twice": the dense accumulator without h_save (GEMM writes x W_acc, the chain adds h B with beta = 1, h hidden), the
  low-rank accumulator (its chain or GEMM pair writes x Q R with a hidden bf16 x Q, then beta = 1), a misaligned dense
  layer (generic GEMM, then the chain with beta = 1).  Checked with check_bound: one ulp of y, one ulp of the first
  product, the hidden rounding's accumulation term.
dX follows the same split (fused dense paths round once, the others twice).
"""
import ctypes
import dataclasses
from typing import Optional

import pytest
import torch

from numerics import (LAMBDA, MAX_INEXACT, UNIT_ROUNDOFF, accumulation_term, bound, check_bound, check_h_save,
                      check_rounded, fp32_floor, rne, to64, ulp)
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
U16, U32 = UNIT_ROUNDOFF[BF16], UNIT_ROUNDOFF[F32]
# f16 subnormals: below 2^-14 an f16 value is held to an absolute spacing of 2^-24, so a hidden f16 rounding (dh, x Q) errs
# by up to 2^-25 however small the value -- a term the relative model u |c| does not cover (bf16 and fp32 reach down to
# 2^-126: nothing to add there)
F16_HALF_SUB = 2.0 ** -25
GUARD = 64                 # guard elements on each side of a view
SENTINEL = -7.25           # exactly representable in both dtypes
WORST = {}                 # (case, stage) -> worst err / limit, printed by the last test
ALLOWED = {}               # (case, stage) -> share of elements allowed off RNE(ref64) (check_rounded stages)


def _dt(dtype):
    return {BF16: _lib.BF16, F16: _lib.F16, F32: _lib.F32}[dtype]


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _sub_term(mult_sq, dt):
    """The subnormal floor of a hidden f16 rounding: sum_k e_k m_k with independent |e_k| <= 2^-25, bounded as in
    accumulation_term by LAMBDA * 2^-25 * sqrt(sum_k m_k^2) (m_k: what each rounded intermediate is multiplied by)."""
    return LAMBDA * F16_HALF_SUB * torch.sqrt(to64(mult_sq))


def _rounded(out, ref, dt, acc, name):
    """check_rounded; in f16 the share of elements allowed off RNE(ref64) grows by the mean of acc / ulp: an fp32 sum
    noise e moves an element across an f16 rounding point with probability ~2 |e| / ulp, and acc (LAMBDA = 4 standard
    deviations of e) over-states that by more than 2x.  An f16 ulp is 8x finer than a bf16 one, so long fp32 sums
    (the generic kernels' K = T chains) reach the 0.5 % of MAX_INEXACT where bf16 sums do not."""
    if dt != F16:
        return dict(check_rounded(out, ref, dt, acc=acc, name=name), allowed=MAX_INEXACT)
    share = float((to64(acc) / ulp(rne(to64(ref), dt), dt)).clamp(max=1.0).mean())
    return dict(check_rounded(out, ref, dt, acc=acc, max_inexact=MAX_INEXACT + share, name=name),
                allowed=MAX_INEXACT + share)


class Arena:
    """The buffers of one call: guarded inputs (NaN neighbours), guarded outputs (sentinel guards, poisonable)."""

    def __init__(self, dtype, misalign=0):
        self.dtype, self.misalign = dtype, misalign
        self.outs = []     # (buf, off, n, view, initial) -- initial: values to restore before a run (grad_beta), or None

    def input(self, t, misalign=None):
        if t is None:
            return None
        off = GUARD + (self.misalign if misalign is None else misalign)
        n = t.numel()
        buf = torch.full((n + off + GUARD,), float("nan"), dtype=self.dtype, device=DEV)
        view = buf[off:off + n].view(t.shape)
        view.copy_(t.to(DEV, self.dtype))
        return view

    def output(self, shape, initial=None, misalign=None):
        off = GUARD + (self.misalign if misalign is None else misalign)
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + off + GUARD,), SENTINEL, dtype=self.dtype, device=DEV)
        view = buf[off:off + n].view(shape)
        self.outs.append((buf, off, n, view, None if initial is None else initial.to(DEV, self.dtype)))
        return view

    def workspace(self, nbytes):
        if not nbytes:
            return None
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
        self.outs.append((ws, 0, ws.numel(), ws, None))
        return ws

    def fill(self, byte):
        """Outputs and workspaces to all-`byte` memory (0xFF = NaN), gradients accumulated onto to their initial values."""
        for buf, off, n, view, init in self.outs:
            if init is not None:
                view.copy_(init)
            elif buf.dtype == torch.uint8:
                buf.fill_(byte)
            else:
                _bits(view).fill_(-1 if byte == 0xFF else 0)

    def check_guards(self, what):
        torch.cuda.synchronize()
        for buf, off, n, view, _ in self.outs:
            if buf.dtype == torch.uint8:
                continue
            lead, trail = buf[:off], buf[off + n:]
            for name, g in (("leading", lead), ("trailing", trail)):
                bad = g != SENTINEL
                assert not bad.any(), f"{what}: {int(bad.sum())} elements of a {name} output guard overwritten"


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@dataclasses.dataclass
class Case:
    name: str
    dtype: torch.dtype
    T: int
    d_in: int
    d_out: int
    r: int
    acc: Optional[str] = None       # None | "dense" | "lowrank"
    r_acc: int = 0
    bias: bool = True
    s: float = 1.0
    grad_beta: float = 0.0
    misalign: int = 0
    switches: dict = dataclasses.field(default_factory=dict)
    y_rounds: str = "once"
    save_h: bool = True              # False: h_save = NULL through the C ABI (forward only)
    seed: int = 0
    dx_rounds: Optional[str] = None  # rounding class of dX when it differs from y's (None: y_rounds)


def _inputs(c: Case):
    g = torch.Generator().manual_seed(1000 + c.seed + c.T + c.r)

    def rnd(*shape, std=1.0):
        return (torch.randn(*shape, generator=g) * std).to(c.dtype)

    d = dict(x=rnd(c.T, c.d_in), A=rnd(c.d_in, c.r, std=0.05), B=rnd(c.r, c.d_out, std=0.05),
             bias=rnd(c.d_out, std=0.1) if c.bias else None, dy=rnd(c.T, c.d_out))
    if c.acc == "dense":
        d["W"] = rnd(c.d_in, c.d_out, std=0.02)
    elif c.acc == "lowrank":
        d["Q"], d["R"] = rnd(c.d_in, c.r_acc, std=0.05), rnd(c.r_acc, c.d_out, std=0.05)
    if c.grad_beta:
        d["dA0"], d["dB0"] = rnd(c.d_in, c.r, std=0.5), rnd(c.r, c.d_out, std=0.5)
        d["dbias0"] = rnd(c.d_out, std=0.5) if c.bias else None
    return d


def _kind(c):
    return {None: _lib.ACC_NONE, "dense": _lib.ACC_DENSE, "lowrank": _lib.ACC_LOWRANK}[c.acc]


def _run_single(c: Case, d, trace=None):
    """Forward then backward through the C ABI, three times (poisoned, zeroed, poisoned); returns the outputs of the
    first run (CPU) after asserting that the three are bit-identical and that no guard was touched.  The workspace sizes
    are queried under the case's switches (the C workspace plan depends on them).  `trace`: a dict that receives the
    ordered kernel names of the third run's forward ("fwd") and backward ("bwd")."""
    with _lib.switch(**c.switches):
        return _run_single_switched(c, d, trace)


def _kernel_seq(fn):
    """Ordered names of the GPU kernels `fn` launches (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]


def _run_single_switched(c: Case, d, trace):
    lib = _lib.load()
    dt, kind = _dt(c.dtype), _kind(c)
    ar = Arena(c.dtype, c.misalign)
    x, A, B, bias, dy = (ar.input(d[k]) for k in ("x", "A", "B", "bias", "dy"))
    acc_down = ar.input(d.get("W", d.get("Q")))
    acc_up = ar.input(d.get("R"))
    hcols = 64 if c.r <= 64 else c.r
    y = ar.output((c.T, c.d_out))
    h = ar.output((c.T, hcols), misalign=0) if c.save_h else None
    fws = ar.workspace(lib.sow_forward_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, dt))
    bwd = c.save_h
    if bwd:
        h_in = ar.input(torch.zeros(c.T, hcols), misalign=0)    # the backward's copy of h_save, NaN neighbours
        dx = ar.output((c.T, c.d_in))
        dA = ar.output((c.d_in, c.r), d.get("dA0"), misalign=0)
        dB = ar.output((c.r, c.d_out), d.get("dB0"), misalign=0)
        dbias = ar.output((c.d_out,), d.get("dbias0"), misalign=0) if c.bias else None
        bws = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, dt))
    runs = []

    def fwd():
        _lib.check(lib.sow_forward(_ptr(x), _ptr(A), _ptr(B), _ptr(acc_down), _ptr(acc_up), _ptr(bias), _ptr(y), _ptr(h),
                                   c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, c.s, dt, _ptr(fws),
                                   0 if fws is None else fws.numel(), _stream()), "sow_forward")

    def bwd_call():
        _lib.check(lib.sow_backward_ex(_ptr(dy), _ptr(x), _ptr(h_in), _ptr(A), _ptr(B), _ptr(acc_down), _ptr(acc_up),
                                       _ptr(dx), _ptr(dA), _ptr(dB), _ptr(dbias), c.T, c.d_in, c.d_out, c.r, c.r_acc,
                                       kind, c.s, c.grad_beta, dt, _ptr(bws), bws.numel(),
                                       _lib.BWD_DATA | _lib.BWD_WEIGHTS, _stream()), "sow_backward_ex")

    for byte in (0xFF, 0x00, 0xFF):
        ar.fill(byte)
        profiled = trace is not None and len(runs) == 2
        if profiled:
            trace["fwd"] = _kernel_seq(fwd)
        else:
            fwd()
        outs = dict(y=y.clone(), h=None if h is None else h.clone())
        if bwd:
            h_in.copy_(h)
            if profiled:
                trace["bwd"] = _kernel_seq(bwd_call)
            else:
                bwd_call()
            outs.update(dx=dx.clone(), dA=dA.clone(), dB=dB.clone(), dbias=None if dbias is None else dbias.clone())
        ar.check_guards(f"{c.name} run {len(runs)}")
        runs.append(outs)
    for k, v in runs[0].items():
        if v is None:
            continue
        for i in (1, 2):
            same = torch.equal(_bits(v), _bits(runs[i][k]))
            assert same, f"{c.name}: {k} of the {'zeroed' if i == 1 else 'repeated'} run differs from the poisoned run"
    return {k: (None if v is None else v.cpu()) for k, v in runs[0].items()}


def _record(c, stage, st):
    WORST[(c.name, stage)] = (st["worst"], st.get("inexact"))
    if "inexact" in st:
        ALLOWED[(c.name, stage)] = st.get("allowed", MAX_INEXACT)


def _check(c: Case, d, out):
    """Stage-by-stage checks of one layer's outputs (float64 references on the CPU)."""
    q = {k: to64(v) for k, v in d.items() if v is not None}
    x, A, B, dy, s = q["x"], q["A"], q["B"], q["dy"], c.s
    T, r = c.T, c.r
    bias = q.get("bias", torch.zeros(c.d_out, dtype=torch.float64))
    xx, AA, BB, dydy = x * x, A * A, B * B, dy * dy
    f32 = c.dtype == F32
    dt = c.dtype
    # ---- h_save
    if c.save_h:
        h_all = to64(out["h"])
        if r <= 64:
            hs, ref = s * (x @ A), s * (x @ A)
            sq = s * s * (xx @ AA)
            st = check_h_save(h_all, ref, r, dt, bnd=bound(ref, dt, accumulation_term(sq, U32, c.d_in)) if f32 else None,
                              acc=None if f32 else fp32_floor(sq, c.d_in), name=f"{c.name}: h_save")
            h = h_all[:, :r]
        else:   # r > 64: the GEMM composition saves x A unscaled, [T, r]
            ref, sq = x @ A, xx @ AA
            st = (check_bound(h_all, ref, bound(ref, dt, accumulation_term(sq, U32, c.d_in)), name=f"{c.name}: h_save")
                  if f32 else _rounded(h_all, ref, dt, fp32_floor(sq, c.d_in), f"{c.name}: h_save"))
            h = s * h_all
        _record(c, "h_save", st)
    else:
        h = None
    # ---- y
    h_vis = h if h is not None else s * (x @ A)         # without h_save: the exact projection (its rounding is hidden)
    hh = h_vis * h_vis
    first = sq_first = None
    hidden = []
    if c.acc == "dense":
        first, sq_first = x @ q["W"], xx @ (q["W"] * q["W"])
    elif c.acc == "lowrank":
        t = x @ q["Q"]
        first, sq_first = t @ q["R"], xx @ (q["Q"] * q["Q"]) @ (q["R"] * q["R"])
        hidden.append(accumulation_term((t * t) @ (q["R"] * q["R"]), UNIT_ROUNDOFF[dt]))   # x Q rounded before . R
        if dt == F16:
            hidden.append(_sub_term((q["R"] * q["R"]).sum(0).expand(c.T, -1), dt))
    y_ref = (first if first is not None else 0) + h_vis @ B + bias
    y_sq = hh @ BB + (sq_first if sq_first is not None else 0)
    n_y = c.d_in + max(r, 64)
    if h is None:
        hidden.append(accumulation_term(hh @ BB, UNIT_ROUNDOFF[dt]))
        if dt == F16:
            hidden.append(_sub_term(BB.sum(0).expand(c.T, -1), dt))
    if f32:
        st = check_bound(out["y"], y_ref, bound(y_ref, dt, accumulation_term(y_sq, U32, n_y), *hidden,
                                                 *([ulp(first, dt)] if first is not None and c.y_rounds == "twice" else [])),
                         name=f"{c.name}: y")
    elif c.y_rounds == "once" and h is not None:
        assert not hidden, f"{c.name}: a path with a hidden rounding cannot be classified as rounding y once"
        st = _rounded(out["y"], y_ref, dt, fp32_floor(y_sq, n_y), f"{c.name}: y")
    else:   # y rounded twice, or once from an h the test cannot see (h_save = NULL)
        first_ulp = [ulp(first, dt)] if first is not None and c.y_rounds == "twice" else []
        st = check_bound(out["y"], y_ref, bound(y_ref, dt, *first_ulp, fp32_floor(y_sq, n_y), *hidden),
                         name=f"{c.name}: y")
    _record(c, "y", st)
    if "dA" not in out:
        return
    # ---- backward
    dh = s * (dy @ B.t())
    dhdh = dh * dh
    u = UNIT_ROUNDOFF[dt]
    gb = c.grad_beta
    # dB, dbias from the visible h_save and dY
    dB_ref = h.t() @ dy + (gb * q["dB0"] if gb else 0)
    dB_sq = hh.t() @ dydy
    if f32:
        st = check_bound(out["dB"], dB_ref, bound(dB_ref, dt, accumulation_term(dB_sq, U32, T)), name=f"{c.name}: dB")
    else:
        st = _rounded(out["dB"], dB_ref, dt, fp32_floor(dB_sq, T), f"{c.name}: dB")
    _record(c, "dB", st)
    if c.bias:
        db_ref = dy.sum(0) + (gb * q["dbias0"] if gb else 0)
        db_sq = dydy.sum(0)
        if f32:
            st = check_bound(out["dbias"], db_ref, bound(db_ref, dt, accumulation_term(db_sq, U32, T)), name=f"{c.name}: dbias")
        else:
            st = _rounded(out["dbias"], db_ref, dt, fp32_floor(db_sq, T), f"{c.name}: dbias")
        _record(c, "dbias", st)
    # dA: dh is internal (bf16: rounded to bf16 before the token reduction)
    dA_ref = x.t() @ dh + (gb * q["dA0"] if gb else 0)
    dA_sq = xx.t() @ dhdh
    sub = [] if dt != F16 else [_sub_term(xx.sum(0)[:, None].expand(-1, r), dt)]
    # fp32: dh is an fp32 sum of d_out terms; where it cancels far below its terms, the error of that sum (not the
    # u |dh| of its rounding) carries into dA and dX -- the accumulation term of the terms s dY_o B_jo themselves
    dh_terms = s * s * (dydy @ BB.t()) if f32 else None
    if f32:
        sub.append(accumulation_term(xx.t() @ dh_terms, U32, c.d_out))
    st = check_bound(out["dA"], dA_ref, bound(dA_ref, dt, accumulation_term(dA_sq, u, T if f32 else 1),
                                              fp32_floor(dA_sq, T), *sub), name=f"{c.name}: dA")
    _record(c, "dA", st)
    if "dx" not in out:   # (shared-input siblings: one summed dX, checked by the caller)
        return
    # dX
    extra = []
    first = None
    if c.acc == "dense":
        first, sq_first = dy @ q["W"].t(), dydy @ (q["W"] * q["W"]).t()
    elif c.acc == "lowrank":
        t = dy @ q["R"].t()
        first, sq_first = t @ q["Q"].t(), dydy @ (q["R"] * q["R"]).t() @ (q["Q"] * q["Q"]).t()
        extra.append(accumulation_term((t * t) @ (q["Q"] * q["Q"]).t(), u))
        if dt == F16:
            extra.append(_sub_term((q["Q"] * q["Q"]).sum(1)[None, :].expand(T, -1), dt))
    if dt == F16:
        extra.append(_sub_term(AA.sum(1)[None, :].expand(T, -1), dt))
    if f32:
        extra.append(accumulation_term(dh_terms @ AA.t(), U32, c.d_out))
    dx_ref = dh @ A.t() + (first if first is not None else 0)
    dx_sq = dhdh @ AA.t() + (sq_first if first is not None else 0)
    n_x = c.d_out + max(r, 64)
    if first is not None and (c.dx_rounds or c.y_rounds) == "twice":
        extra.append(ulp(first, dt))
    st = check_bound(out["dx"], dx_ref, bound(dx_ref, dt, accumulation_term(dhdh @ AA.t(), u, n_x if f32 else 1),
                                              fp32_floor(dx_sq, n_x), *extra), name=f"{c.name}: dx")
    _record(c, "dx", st)


# Each recipe names the path it reaches, read off the *_supported predicates and the dispatch of api.hip.
CASES = [
    # chain2 streaming forward / backward (chain2_supported: bf16, r even in [4, 64], widths % 8, 16-byte views, T >= 64;
    # T / 64 > SHORT_NTB = 128 token blocks, so no short split) + tn_partial_dma_wide + tn_reduce
    Case("chain2_T8193", BF16, 8193, 512, 264, 50, s=0.5),
    Case("chain2_T32769_r64_colsum", BF16, 32769, 256, 520, 64),          # r = 64: dbias by colsum_kernel (api.hip: backward_impl)
    Case("chain2_T32769_grad_beta", BF16, 32769, 256, 264, 50, bias=True, s=0.5, grad_beta=1.0),
    # chain_short: T / 64 <= 128 token blocks and nst + nsl >= 24 column tiles: phase 1 split over K + h_reduce, phase 2
    # split over the output columns
    Case("chain_short_T65", BF16, 65, 1024, 1032, 50),
    Case("chain_short_T1000", BF16, 1000, 1024, 1032, 16, s=0.5, bias=False),
    # generic chain (launch_chain_t) / generic tn_partial: r odd or < 4, T < 64, widths not % 8, misaligned views
    Case("generic_r63_T4097", BF16, 4097, 512, 264, 63, s=0.5),           # r = 63: the ones column is the last free one
    Case("generic_T1_r1", BF16, 1, 64, 72, 1),
    Case("generic_T63_r2_dout100", BF16, 63, 256, 100, 2, s=0.5),
    Case("generic_din301_r1", BF16, 4097, 301, 264, 1, bias=False),
    Case("generic_misaligned_bf16", BF16, 8193, 512, 264, 50, misalign=1, s=0.5),
    # dense accumulator, r <= 64: gemm4h (<= 2 column tiles of 256, >= 120 tiles: T = 32769 -> 129 x 2)
    Case("gemm4h_T32769", BF16, 32769, 512, 264, 50, acc="dense", s=0.5),
    # gemm2h: the same shape with gemm4h switched off (gemm2h_supported: <= 2 column tiles, >= 160 tiles)
    Case("gemm2h_T32769", BF16, 32769, 512, 264, 50, acc="dense", switches=dict(NO_GEMM4H=1)),
    # d_out > 512 at short T: chain_short (H only) + gemm2 with the rank extension, split over K through the workspace
    # (gemm4_split_plan: <= 128 output tiles and >= 96 K-tiles of 64, so d_in = 6144; at d_in = 4096 the same layer runs
    # gemm3s unsplit; the backward's K = d_out = 4096 runs gemm3s)
    Case("dense_short_splitk", BF16, 1024, 6144, 4096, 16, acc="dense", s=0.5),
    # dense accumulator with h_save = NULL (allowed by the C ABI): gemm_auto writes x W_acc, the chain adds h B (beta = 1)
    Case("dense_without_h", BF16, 8193, 512, 264, 50, acc="dense", save_h=False, y_rounds="twice"),
    # misaligned dense layer: gemm4h / gemm2h / gemm2 reject the views -> generic GEMM + generic chain with beta = 1
    Case("dense_misaligned", BF16, 4097, 512, 264, 50, acc="dense", misalign=1, y_rounds="twice"),
    # r > 64: GEMM composition (h = x A unscaled in h_save [T, r], y = s h B + bias)
    Case("wide_r96", BF16, 4097, 512, 264, 96, s=0.5),
    # low-rank accumulator: r_acc <= 64 through the chain kernel (scale 1) then the live chain with beta = 1; r_acc > 64
    # through two GEMMs and the workspace's [T, r_acc] intermediate
    Case("lowrank_racc32", BF16, 8193, 512, 264, 50, acc="lowrank", r_acc=32, y_rounds="twice"),
    Case("lowrank_racc96", BF16, 4097, 512, 264, 50, acc="lowrank", r_acc=96, s=0.5, y_rounds="twice"),
    # fp32: chain3f + planes pre-pass (T >= 8192, workspace planes); tn_partial_f32_quad (T >= 4096, >= 3 column groups)
    Case("chain3f_T8193", F32, 8193, 256, 264, 50, s=0.5),
    Case("chain3f_lowrank_racc32", F32, 8193, 256, 264, 50, acc="lowrank", r_acc=32, y_rounds="twice"),
    # chain2f: short T (K / column split, nst + nsl >= 24) and the F32_EXACT switch at long T
    Case("chain2f_short_T1000", F32, 1000, 1024, 1032, 16),
    Case("chain2f_exact_T8193", F32, 8193, 256, 264, 50, s=0.5, switches=dict(F32_EXACT=1)),
    # tn_partial_dma_f32_wide: fewer than 3 column groups per operand
    Case("tn_f32_wide_T8193", F32, 8193, 128, 128, 16),
    # gemm_x3: fp32 dense accumulator (gemm_auto -> launch_gemm) then the chain with beta = 1
    Case("gemm_x3_dense_f32", F32, 4097, 256, 264, 16, acc="dense", y_rounds="twice"),
    Case("generic_misaligned_f32", F32, 8193, 256, 264, 50, misalign=1),
    Case("generic_T65_f32_r1", F32, 65, 256, 72, 1, s=0.5),
    # found by the random sweep (test_gpu_fuzz_elementwise.py): r = 1, d_out = 80 -- dh = s dY B^T cancels to ~1/1000 of
    # its terms in many rows, and the fp32 error of that sum, not of its rounding, dominates dX and dA
    Case("generic_f32_T4618_304x80_r1", F32, 4618, 304, 80, 1, bias=False, s=2.0, grad_beta=0.5, seed=93),
]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_layer_path(c):
    d = _inputs(c)
    out = _run_single(c, d)
    _check(c, d, out)


def _has_kernel(seq, kernel):
    # demangled ("sow::chain_kernel<...>") or mangled ("_ZN3sow12chain_kernel...") names of exactly this kernel
    return any(f"sow::{kernel}" in n or f"{len(kernel)}{kernel}" in n for n in seq)


# Dispatch switches (api.hip): (case, kernels the trace must show, kernels it must not).  The rounding class of
# each is read off the path the switch leaves:
# * NO_SHORT_SPLIT: launch_chain_short declines (api.hip), the layer (no accumulator) runs the unsplit chain: y and dX
#   are still written by one kernel from operands the test sees ("once");
# * FORCE_GEMM_V1: gemm4h / gemm2h / gemm2 all decline, gemm_auto takes the generic kernel for x W_acc and dY W_acc^T and
#   the chain adds the low-rank term with beta = 1 ("twice", as dense_misaligned);
# * NO_GEMM3S: a dense layer with fewer than 160 tiles of 256 x 256 fails the bf16 gate of pick_gemm (api.hip) and takes the
#   same generic composition ("twice"); without the switch its >= 96 tiles of 128 x 128 run gemm3s_kernel.
_FAST_GEMMS = ("gemm2_kernel", "gemm2h_kernel", "gemm3_kernel", "gemm3s_kernel", "gemm4_kernel", "gemm4_f16_kernel")
SWITCHED = [
    (Case("no_short_split_bf16", BF16, 700, 1024, 1536, 50, s=0.5, switches=dict(NO_SHORT_SPLIT=1)), ("chain2_kernel",), ("h_reduce_kernel",)),
    (Case("no_short_split_f32", F32, 700, 1024, 1536, 50, s=0.5, switches=dict(NO_SHORT_SPLIT=1)), (), ("h_reduce_kernel",)),
    (Case("force_gemm_v1_dense", BF16, 4097, 512, 264, 50, acc="dense", switches=dict(FORCE_GEMM_V1=1), y_rounds="twice"),
     ("gemm_kernel",), _FAST_GEMMS),
    (Case("no_gemm3s_dense_short", BF16, 1800, 1024, 1800, 16, acc="dense", s=0.5, switches=dict(NO_GEMM3S=1), y_rounds="twice"),
     ("gemm_kernel",), ("gemm3s_kernel",)),
]


@pytest.mark.parametrize("c,present,absent", SWITCHED, ids=[s[0].name for s in SWITCHED])
def test_switched_layer_path(c, present, absent):
    d = _inputs(c)
    trace = {}
    out = _run_single(c, d, trace)
    seq = trace["fwd"] + trace["bwd"]
    for k in present:
        assert _has_kernel(seq, k), f"{c.name}: no {k} in {sorted(set(seq))}"
    for k in absent:
        assert not _has_kernel(seq, k), f"{c.name}: {k} ran under {c.switches}: {sorted(set(seq))}"
    _check(c, d, out)


def test_short_split_and_gemm3s_are_the_defaults_the_switches_replace():
    """The two shapes above without their switch: the short split's h_reduce_kernel and gemm3s_kernel do run by default, so
    the switched cases take another path than the unswitched ones."""
    for (c, _, absent) in (SWITCHED[0], SWITCHED[3]):
        trace = {}
        _run_single(dataclasses.replace(c, switches={}), _inputs(c), trace)
        assert _has_kernel(trace["fwd"] + trace["bwd"], absent[0]), f"{c.name}: {absent[0]} is not the default path"


# ---- grouped calls: sow_forward_group shares chain2 launches; sow_backward_group with DATA | WEIGHTS plans the row-owner
# weight-gradient kernel (tn_partial_rows) over the group (group_rows_plan: bf16, widths % 8, 16-byte views, r <= 63
# with a bias)
# with a bias); a group too small to fill one resident round with slabs of >= 512 tokens (three layers at T = 8193) keeps
# the column-owner kernel, grouped (launch_tn_group).  name -> (layers, row-owner kernel expected)
GROUPS = [
    ("group3_T8193", [Case("g0", BF16, 8193, 256, 264, 50, s=0.5), Case("g1", BF16, 8193, 256, 512, 16, bias=False),
                      Case("g2", BF16, 8193, 256, 136, 8)], False),
    ("group4_T32769_rows", [Case("g0", BF16, 32769, 256, 264, 50), Case("g1", BF16, 32769, 256, 256, 16, bias=False, s=0.5),
                            Case("g2", BF16, 32769, 256, 264, 8), Case("g3", BF16, 32769, 256, 256, 64, bias=False)], True),
]


@pytest.mark.parametrize("name,layers,rows", GROUPS, ids=[g[0] for g in GROUPS])
def test_grouped_path(name, layers, rows):
    lib = _lib.load()
    layers = [dataclasses.replace(c, name=f"{name}.{c.name}", seed=i) for i, c in enumerate(layers)]
    data = [_inputs(c) for c in layers]
    ar = Arena(BF16)
    arr = (_lib.LayerArgs * len(layers))()
    bufs = []
    for i, (c, d) in enumerate(zip(layers, data)):
        b = dict(x=ar.input(d["x"]), A=ar.input(d["A"]), B=ar.input(d["B"]), bias=ar.input(d["bias"]), dy=ar.input(d["dy"]),
                 y=ar.output((c.T, c.d_out)), h=ar.output((c.T, 64)), dx=ar.output((c.T, c.d_in)),
                 dA=ar.output((c.d_in, c.r)), dB=ar.output((c.r, c.d_out)), dbias=ar.output((c.d_out,)) if c.bias else None)
        b["ws"] = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, _lib.ACC_NONE, _lib.BF16))
        bufs.append(b)
        arr[i] = _lib.LayerArgs(x=_ptr(b["x"]), A=_ptr(b["A"]), B=_ptr(b["B"]), acc_down=None, acc_up=None,
                                bias=_ptr(b["bias"]), y=_ptr(b["y"]), h_save=_ptr(b["h"]), dy=_ptr(b["dy"]), dx=_ptr(b["dx"]),
                                dA=_ptr(b["dA"]), dB=_ptr(b["dB"]), dbias=_ptr(b["dbias"]), T=c.T, d_in=c.d_in, d_out=c.d_out,
                                r_live=c.r, r_acc=0, acc_kind=_lib.ACC_NONE, scale=c.s, grad_beta=0.0,
                                workspace=_ptr(b["ws"]), workspace_bytes=b["ws"].numel())
    slabs = ctypes.c_int * (2 * len(layers))
    assert lib.sow_backward_group_plan(arr, len(layers), _lib.BF16, _lib.BWD_DATA | _lib.BWD_WEIGHTS, slabs()) == int(rows)
    keys = ("y", "h", "dx", "dA", "dB", "dbias")
    runs = []
    for byte in (0xFF, 0x00, 0xFF):
        ar.fill(byte)
        _lib.check(lib.sow_forward_group(arr, len(layers), _lib.BF16, _stream()), "sow_forward_group")
        _lib.check(lib.sow_backward_group(arr, len(layers), _lib.BF16, _lib.BWD_DATA | _lib.BWD_WEIGHTS, _stream()),
                   "sow_backward_group")
        ar.check_guards(f"{name} run {len(runs)}")
        runs.append([{k: (None if b[k] is None else b[k].clone()) for k in keys} for b in bufs])
    for i, c in enumerate(layers):
        for k in keys:
            if runs[0][i][k] is not None:
                assert torch.equal(_bits(runs[0][i][k]), _bits(runs[1][i][k])), f"{c.name}: {k} differs on zeroed memory"
                assert torch.equal(_bits(runs[0][i][k]), _bits(runs[2][i][k])), f"{c.name}: {k} differs on a repeat"
        _check(c, data[i], {k: (None if v is None else v.cpu()) for k, v in runs[0][i].items()})


# ---- sow_gemm: C = alpha op(A) op(B) + beta C + bias (one rounding of an fp32 sum)
GEMMS = [
    # gemm4 streaming: the bf16 gate of pick_gemm and >= 120 tiles of 256 x 256 (32 x 6)
    ("gemm4_stream", 8192, 1376, 512, True, 0.0, False),
    # gemm3s: fewer than 160 big tiles, >= 96 tiles of 128 x 128 and K >= 512 (no workspace, so no split)
    ("gemm3s_beta1", 4096, 1024, 1024, True, 1.0, False),
    # split-K gemm4 through the workspace (sow_gemm_workspace_bytes > 0: <= 128 tiles, >= 96 K-tiles): 32 tiles x 4 splits
    ("gemm4_splitk", 1024, 2048, 6144, False, 0.0, True),
    # generic kernel: N not a multiple of 8
    ("gemm_generic_N1001", 1000, 1001, 300, True, 0.0, False),
]


@pytest.mark.parametrize("name,M,N,K,has_bias,beta,use_ws", GEMMS, ids=[g[0] for g in GEMMS])
def test_gemm_path(name, M, N, K, has_bias, beta, use_ws):
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = (torch.randn(K, N, generator=g) * 0.05).bfloat16()
    bias = (torch.randn(N, generator=g) * 0.1).bfloat16() if has_bias else None
    c0 = torch.randn(M, N, generator=g).bfloat16() if beta else None
    out = _run_gemm(name, a, b, bias, c0, beta, use_ws)
    a64, b64 = to64(a), to64(b)
    ref = a64 @ b64 + (to64(bias) if has_bias else 0) + (beta * to64(c0) if beta else 0)
    st = check_rounded(out, ref, BF16, acc=fp32_floor((a64 * a64) @ (b64 * b64), K), name=name)
    WORST[(name, "C")] = (st["worst"], st["inexact"])


def test_gemm_force_v1():
    """FORCE_GEMM_V1 = 1 on a shape whose 176 tiles of 128 x 128 take gemm3s by default: sow_gemm_ex runs the generic kernel alone."""
    name, M, N, K = "gemm_force_v1", 2048, 1376, 512
    g = torch.Generator().manual_seed(M + N + K + 1)
    a = torch.randn(M, K, generator=g).bfloat16()
    b = (torch.randn(K, N, generator=g) * 0.05).bfloat16()
    bias = (torch.randn(N, generator=g) * 0.1).bfloat16()
    trace = []
    with _lib.switch(FORCE_GEMM_V1=1):
        out = _run_gemm(name, a, b, bias, None, 0.0, False, trace=trace)
    assert _has_kernel(trace, "gemm_kernel") and not any(_has_kernel(trace, k) for k in _FAST_GEMMS), sorted(set(trace))
    a64, b64 = to64(a), to64(b)
    st = check_rounded(out, a64 @ b64 + to64(bias), BF16, acc=fp32_floor((a64 * a64) @ (b64 * b64), K), name=name)
    WORST[(name, "C")] = (st["worst"], st["inexact"])


def _run_gemm(name, a, b, bias, c0, beta, use_ws, trace=None):
    """bf16 sow_gemm_ex C = a b + beta C0 + bias on the given operands (a [M, K], b [K, N], bias [N] or None, C0 [M, N] or
    None): three bit-identical runs with intact guards; C of the first on the CPU.  `trace`: a list that receives the kernel
    names of the third run."""
    lib = _lib.load()
    (M, K), N = a.shape, b.shape[1]
    ar = Arena(BF16)
    A, B, Bi = ar.input(a), ar.input(b), ar.input(bias)
    C = ar.output((M, N), c0)
    nws = lib.sow_gemm_workspace_bytes(M, N, K, 0, _lib.BF16) if use_ws else 0
    assert (nws > 0) == use_ws
    ws = ar.workspace(nws)
    runs = []
    for byte in (0xFF, 0x00, 0xFF):
        ar.fill(byte)
        call = lambda: _lib.check(lib.sow_gemm_ex(_ptr(A), K, 0, _ptr(B), N, 0, _ptr(C), N, _ptr(Bi), M, N, K, 1.0, beta,
                                                  _lib.BF16, _ptr(ws), nws, _stream()), "sow_gemm_ex")
        if trace is not None and len(runs) == 2:
            trace += _kernel_seq(call)
        else:
            call()
        ar.check_guards(f"{name} run {len(runs)}")
        runs.append(C.clone())
    assert torch.equal(_bits(runs[0]), _bits(runs[1])) and torch.equal(_bits(runs[0]), _bits(runs[2]))
    return runs[0].cpu()


def test_zz_report_worst_ratios():
    """Prints the worst err / limit (and for check_rounded the share of elements not equal to RNE(ref64)) of every checked
    stage of this module's cases (run with -s to see it)."""
    for (case, stage), (w, inexact) in sorted(WORST.items()):
        print(f"worst err/limit {case:34s} {stage:7s} {w:.3f}" + ("" if inexact is None else f"  inexact {100 * inexact:.4f} %"))
