"""The device gradient record on the GPU: sow_grad_stats_flat (sum of squares in double, coefficient, multiplier, non-finite
flag), sow_adamw_flat_seg_stats (AdamW that reads its multiplier and its go / no-go flag from the record),
FactorAdamW.step's clipping / skipping keywords, sow_amd.clip_grad_norm_, one HIP-graph capture of the whole step, and
the zero padding of the flat gradient that the sum relies on.

Bounds.  sumsq: |got - ref| <= max(n, 1) 2^-52 ref, ref the float64 sum of the float64 squares of the stored values
(grad_stats_ref.sumsq_bound: any two summation orders of n non-negative doubles, squares exact).  fp32 fields: one fp32 ulp
of the float64 formula.  AdamW: step_numerics.check_step against float64 AdamW with grad_scale set to the fp32 grad_mult
the record holds (the kernel's own operand); that grad_mult is held against the float64 clip formula separately."""
import ctypes
import math
import struct

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import grad_stats_ref as R
from step_numerics import adamw_ref, check_step
from sow_amd import FactorAdamW, FactorBucket, SoWLinear, _lib, clip_grad_norm_, factor_parameters, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: _lib.F32, BF16: _lib.BF16, F16: _lib.F16}
INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
DTYPES = [F32, BF16, F16]
DIDS = ["f32", "bf16", "f16"]
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]
PIDS = ["f32-f32", "bf16-bf16", "bf16-f32", "f16-f16", "f16-f32"]
BETAS, EPS = (0.9, 0.999), 1e-8
SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 512, 2048 * 1024 + 8, 3 * 2 ** 20 + 5]
NMAX = max(SIZES) + 1


def _bits(t):
    return t.view(INT[t.dtype])


def _s():
    return torch.cuda.current_stream().cuda_stream


def _rec(st) -> dict:
    """The record read back (synchronises): the six fields by name."""
    raw = bytes(st.buf.cpu().numpy().tobytes())
    return dict(zip(("sumsq", "total_sq", "total_norm", "clip_coef", "grad_mult", "nonfinite"), struct.unpack("<ddfffi", raw)))


def _raw_stats(grad, n, dtype, ws, out, *, gs=1.0, max_norm=0.0, extra=None, ls=None, finf=None, cnt=None, ws_bytes=None):
    lib = _lib.load()
    return lib.sow_grad_stats_flat(grad.data_ptr() if n else None, n, DT[dtype], gs, max_norm,
                                   None if extra is None else extra.data_ptr(), None if ls is None else ls.data_ptr(),
                                   None if finf is None else finf.data_ptr(), None if cnt is None else cnt.data_ptr(),
                                   0 if cnt is None else cnt.numel(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                   out.data_ptr(), _s())


_BASE: dict = {}


def _base(dtype, kind):
    """NMAX elements on the CPU (float64 of the stored values) and on the GPU, built once per dtype and kind.
    gauss: N(0, 1) times one magnitude per block of 1024 elements, 2^-20 .. 2^10; exact: integers in [-8, 8] times 2^-3."""
    key = (dtype, kind)
    if key not in _BASE:
        g = torch.Generator().manual_seed(len(_BASE) + 1)
        if kind == "gauss":
            mag = torch.randint(-20, 11, ((NMAX + 1023) // 1024,), generator=g).double().exp2().repeat_interleave(1024)[:NMAX]
            host = (torch.randn(NMAX, generator=g, dtype=torch.float64) * mag).to(dtype)
        else:
            host = (torch.randint(-8, 9, (NMAX,), generator=g).double() * 0.125).to(dtype)
        _BASE[key] = (host.double(), host.to(DEV))
    return _BASE[key]


# ------------------------------------------------------------------------------------------------ 1. sum of squares
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "odd-pointer"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_sum_of_squares(dtype, off):
    lib = _lib.load()
    for kind in ("gauss", "exact"):
        host64, dev = _base(dtype, kind)
        for n in SIZES:
            g = dev[off:off + n]
            assert n == 0 or (g.data_ptr() % 16 == 0) == (off == 0)
            ws = torch.empty(lib.sow_grad_stats_workspace_bytes(n), dtype=torch.uint8, device=DEV)
            outs = [torch.empty(32, dtype=torch.uint8, device=DEV) for _ in range(3)]
            for o in outs:
                _lib.check(_raw_stats(g, n, dtype, ws, o), "sow_grad_stats_flat")
            raws = [bytes(o.cpu().numpy().tobytes()) for o in outs]
            assert raws[0] == raws[1] == raws[2], f"{kind} n={n}: three calls, different bits"
            got = struct.unpack("<ddfffi", raws[0])
            ref = float(host64[off:off + n].square().sum())
            err = abs(got[0] - ref)
            print(f"{kind} {dtype} n={n} off={off}: sumsq {got[0]!r} ref {ref!r} err {err:.3g} bound {R.sumsq_bound(n, ref):.3g}")
            if kind == "exact":
                assert got[0] == ref, f"exact data n={n}: {got[0]!r} != {ref!r}"
            else:
                assert err <= R.sumsq_bound(n, ref), f"gauss n={n}: |{got[0]!r} - {ref!r}| = {err:.3g}"
            assert got[1] == got[0] and got[3] == 1.0 and got[4] == 1.0 and got[5] == 0
            assert R.within_f32_ulps(got[2], math.sqrt(ref))


def test_alignment_does_not_change_the_bits():
    """The same values behind a 16-byte-aligned pointer and behind an odd one: the same sumsq, bit for bit."""
    for dtype in DTYPES:
        _, dev = _base(dtype, "gauss")
        for n in (9, 2049, 2048 * 1024 + 8):
            moved = torch.empty(n + 1, dtype=dtype, device=DEV)
            moved[1:].copy_(dev[:n])
            a = ops.grad_stats_flat(dev[:n])
            b = ops.grad_stats_flat(moved[1:])
            assert moved[1:].data_ptr() % 16 != 0
            assert _rec(a)["sumsq"] == _rec(b)["sumsq"], (dtype, n)


# ------------------------------------------------------------------------------------------------ 2. poison
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_poisoned_workspace_and_record(dtype):
    lib = _lib.load()
    _, dev = _base(dtype, "gauss")
    for n in (0, 9, 2049, 2048 * 1024 + 8):
        need = lib.sow_grad_stats_workspace_bytes(n)
        res = []
        for fill in (0x00, 0xFF):
            ws = torch.full((need + 64,), fill, dtype=torch.uint8, device=DEV)
            out = torch.full((32 + 64,), fill, dtype=torch.uint8, device=DEV)
            _lib.check(_raw_stats(dev[:n], n, dtype, ws, out, ws_bytes=need), "sow_grad_stats_flat")
            res.append(bytes(out[:32].cpu().numpy().tobytes()))
            assert bool((out[32:] == fill).all()) and bool((ws[need:] == fill).all()), "wrote past the record or the workspace"
        assert res[0] == res[1], f"n={n}: the result depends on what the workspace or the record held"
        out = torch.full((32,), 0xFF, dtype=torch.uint8, device=DEV)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        assert _raw_stats(dev[:n], n, dtype, ws, out, ws_bytes=need - 1) == _lib.ERR_WORKSPACE
        torch.cuda.synchronize()
        assert bool((out == 0xFF).all()) and bool((ws == 0xFF).all())


# ------------------------------------------------------------------------------------------------ 3. non-finite
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_one_non_finite_element_sets_the_flag(dtype):
    n = 2048 * 2 + 13
    _, dev = _base(dtype, "gauss")
    flags, what = [], []
    for off in (0, 1):
        buf = dev[off:off + n].clone() if off == 0 else torch.empty(n + 1, dtype=dtype, device=DEV)[1:].copy_(dev[1:1 + n])
        for pos in (0, n - 1, n - 3, 5, 2048 + 3, n // 2):          # first, last, tail, head, second tile, middle
            for val in (math.inf, -math.inf, math.nan):
                keep = buf[pos].clone()
                buf[pos] = val
                flags.append(ops.grad_stats_flat(buf).nonfinite.clone())
                what.append((off, pos, val))
                buf[pos] = keep
        flags.append(1 - ops.grad_stats_flat(buf).nonfinite.clone())     # and without one it is clear
        what.append((off, "none", 0.0))
    got = torch.stack(flags).cpu().tolist()
    assert all(f == 1 for f in got), [w for w, f in zip(what, got) if f != 1]


def test_large_finite_values_are_not_an_overflow():
    for dtype, val, n in ((F16, 65504.0, 2048 * 3 + 5), (F32, 3e38, 2048 * 3 + 5), (F32, 3e38, 2048 * 1024 + 8)):
        buf = torch.full((n,), val, dtype=dtype, device=DEV)
        r = _rec(ops.grad_stats_flat(buf))
        ref = R.sumsq(buf.cpu())                    # the float64 sum of the float64 squares of the stored values
        assert r["nonfinite"] == 0 and math.isfinite(r["sumsq"]) and math.isfinite(ref)
        assert abs(r["sumsq"] - ref) <= R.sumsq_bound(n, ref), (dtype, n, r["sumsq"], ref)
        # an fp32 total_norm may overflow to inf; the flag looks at the double
        assert r["total_sq"] == r["sumsq"]


def test_found_inf_alone_sets_the_flag():
    _, dev = _base(F32, "gauss")
    cnt = torch.tensor([0, 5, 0], dtype=torch.int32, device=DEV)
    for finf, want in ((0.0, 0), (1.0, 1), (2.0, 1)):
        st = ops.grad_stats_flat(dev[:5000], found_inf=torch.tensor([finf], device=DEV), skip_counters=cnt)
        r = _rec(st)
        assert r["nonfinite"] == want and math.isfinite(r["total_sq"])
    assert cnt.cpu().tolist() == [2, 7, 2]


# ------------------------------------------------------------------------------------------------ 4. coefficient, multiplier
@pytest.mark.parametrize("dtype", DTYPES, ids=DIDS)
def test_clip_coefficient_and_gradient_multiplier(dtype):
    n = 2048 * 5 + 77
    host64, dev = _base(dtype, "gauss")
    g = dev[:n]
    sq = float(host64[:n].square().sum())
    norm = math.sqrt(sq)
    for mx in (None, 0.0, math.inf, norm * 1.5, norm * (1 + 1e-3)):
        r = _rec(ops.grad_stats_flat(g, max_norm=mx))
        assert r["clip_coef"] == 1.0 and r["grad_mult"] == 1.0, mx
    for mx in (norm * 0.99, norm / 7.0, 1e-3 * norm):
        for gs in (1.0, 0.37):
            for ls_host, ls_dev in ((None, None), (1024.0, None), (None, 1024.0), (3.0, None), (None, 3.0)):
                for extra in (None, 0.3 * sq):
                    ls = ls_host if ls_host is not None else (torch.tensor([ls_dev], device=DEV) if ls_dev is not None else None)
                    lsv = ls_host or ls_dev or 1.0
                    # a host loss scale is folded into the fp32 grad_scale argument: the kernel sees that rounded quotient
                    gs_seen = float(torch.tensor(gs / lsv, dtype=F32)) if ls_host is not None else float(torch.tensor(gs, dtype=F32))
                    ls_seen = 1.0 if ls_host is not None else float(torch.tensor(lsv, dtype=F32))
                    ex = None if extra is None else torch.tensor([extra], dtype=torch.float64, device=DEV)
                    r = _rec(ops.grad_stats_flat(g, grad_scale=gs, max_norm=mx * gs / lsv, extra_sq_norm=ex, loss_scale=ls))
                    ref = R.record(sq, grad_scale=gs_seen, loss_scale=ls_seen, max_norm=float(torch.tensor(mx * gs / lsv, dtype=F32)),
                                   extra_sq=extra or 0.0)
                    tag = (mx, gs, ls_host, ls_dev, extra)
                    assert abs(r["total_sq"] - ref["total_sq"]) <= (n + 4) * 2.0 ** -52 * ref["total_sq"], tag
                    assert R.within_f32_ulps(r["total_norm"], ref["total_norm"]), tag
                    assert R.within_f32_ulps(r["clip_coef"], ref["clip_coef"]), tag
                    assert R.within_f32_ulps(r["grad_mult"], ref["grad_mult"]), tag
                    assert (r["clip_coef"] < 1.0) == (ref["clip_coef"] < 1.0) and r["nonfinite"] == 0, tag


# ------------------------------------------------------------------------------------------------ 5. AdamW with the record
GUARD = 64
SEG_LEN = (300, 1000, 777)
SEG_HP = ((1e-2, 0.1, 1), (3e-4, 0.0, 7), (1e-3, 0.05, 1000))      # lr, weight decay, step


def _data(n, pdtype, sdtype, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g, dtype=torch.float64) * 0.05).to(pdtype)
    gr = torch.randn(n, generator=g, dtype=torch.float64) * 1e-2
    t = n // 4
    gr[:t] = 0.0
    gr[t:2 * t] *= 1e-6
    gr[3 * t:] *= 1e4 if pdtype != F16 else 1e3
    m = (torch.randn(n, generator=g, dtype=torch.float64) * 1e-3).to(sdtype)
    v = (torch.rand(n, generator=g, dtype=torch.float64) * 1e-4).to(sdtype)
    return p, gr.to(pdtype), m, v


def _nan_fill(t):
    n = t.numel()
    if t.dtype == F32:
        _bits(t).copy_((0x7FC00001 + torch.arange(n, device=t.device) % 4096).to(torch.int32))
    else:
        base = 0x7FC1 if t.dtype == BF16 else 0x7E01
        _bits(t).copy_((base + torch.arange(n, device=t.device) % 32).to(torch.int16))
    return t


def _layout():
    b0 = GUARD
    b1 = b0 + SEG_LEN[0]
    b2 = b1 + SEG_LEN[1] + 64
    total = b2 + SEG_LEN[2] + GUARD
    return [(b0, b1), (b1, b1 + SEG_LEN[1]), (b2, b2 + SEG_LEN[2])], total


def _segment_buffers(pdtype, sdtype, hp=SEG_HP, zero_moments=False):
    """p, g, m, v over guard | segment 0 | segment 1 | gap | segment 2 | guard, NaN outside the segments; `live` marks them."""
    ranges, total = _layout()
    host = _data(total, pdtype, sdtype, seed=3)
    bufs = [_nan_fill(torch.empty(total, dtype=t.dtype, device=DEV)) for t in host]
    live = torch.zeros(total, dtype=torch.bool, device=DEV)
    for (b, e), (_, _, step) in zip(ranges, hp):
        live[b:e] = True
        for buf, t in zip(bufs, host):
            buf[b:e].copy_(t[b:e])
        if step == 1 or zero_moments:
            bufs[2][b:e].zero_()
            bufs[3][b:e].zero_()
    return ranges, bufs, live


def _live_gradient(bufs, ranges):
    """The gradients of the segments as one contiguous finite buffer (the record is taken over this one)."""
    return torch.cat([bufs[1][b:e] for b, e in ranges])


def _stats_step(bufs, rows, st, pdtype, sdtype, cnt_idx=None, counters=None, skip=0):
    lib = _lib.load()
    arr = (_lib.AdamwSegment * len(rows))(*[_lib.AdamwSegment(*r) for r in rows])
    ci = None if cnt_idx is None else (ctypes.c_int * len(rows))(*cnt_idx)
    return lib.sow_adamw_flat_seg_stats(*[b.data_ptr() for b in bufs], arr, ci, len(rows), BETAS[0], BETAS[1], EPS,
                                        st.buf.data_ptr(), skip, None if counters is None else counters.data_ptr(),
                                        0 if counters is None else counters.numel(), DT[pdtype], DT[sdtype], _s())


def _check_segments(bufs, before, ranges, hp, gm, pdtype, sdtype, name, steps=None):
    for k, ((b, e), (lr, wd, step)) in enumerate(zip(ranges, hp)):
        p0, g0, m0, v0 = (t[b:e].cpu() for t in before)
        refs, mags = adamw_ref(p0, g0, m0, v0, lr=lr, betas=BETAS, eps=EPS, wd=wd, step=steps[k] if steps else step, grad_scale=gm)
        out = dict(p=bufs[0][b:e].cpu(), m=bufs[2][b:e].cpu(), v=bufs[3][b:e].cpu())
        stats = check_step(out, refs, mags, pdtype, sdtype, f"{name} segment {k}")
        print(f"{name} segment {k} {pdtype}/{sdtype}: " + ", ".join(f"{q} {s['worst']:.3g}" for q, s in stats.items()))


def _gaps_untouched(bufs, before, live, name):
    for nm, buf, old in zip("pgmv", bufs, before):
        same = _bits(buf) == _bits(old)
        assert bool(same[~live].all()), f"{name}: {nm} was rewritten outside every segment"
    assert torch.equal(_bits(bufs[1]), _bits(before[1])), f"{name}: the gradient is read only"


@pytest.mark.parametrize("pdtype,sdtype", PAIRS, ids=PIDS)
def test_adamw_unclipped_equals_flat_seg_bit_for_bit(pdtype, sdtype):
    lib = _lib.load()
    ranges, bufs, live = _segment_buffers(pdtype, sdtype)
    twin = [b.clone() for b in bufs]
    before = [b.clone() for b in bufs]
    rows = [(b, e, lr, wd, step) for (b, e), (lr, wd, step) in zip(ranges, SEG_HP)]
    st = ops.grad_stats_flat(_live_gradient(bufs, ranges), grad_scale=0.5)
    assert _rec(st)["grad_mult"] == 0.5 and _rec(st)["clip_coef"] == 1.0
    _lib.check(_stats_step(bufs, rows, st, pdtype, sdtype), "sow_adamw_flat_seg_stats")
    arr = (_lib.AdamwSegment * len(rows))(*[_lib.AdamwSegment(*r) for r in rows])
    _lib.check(lib.sow_adamw_flat_seg(*[b.data_ptr() for b in twin], arr, len(rows), BETAS[0], BETAS[1], EPS, 0.5, DT[pdtype],
                                      DT[sdtype], _s()), "sow_adamw_flat_seg")
    torch.cuda.synchronize()
    for nm, a, b in zip("pgmv", bufs, twin):
        assert torch.equal(_bits(a), _bits(b)), f"{nm}: differs from sow_adamw_flat_seg"
    _gaps_untouched(bufs, before, live, "unclipped")
    assert not torch.equal(_bits(bufs[0]), _bits(before[0]))


@pytest.mark.parametrize("pdtype,sdtype", PAIRS, ids=PIDS)
def test_adamw_clipped_against_fp64(pdtype, sdtype):
    ranges, bufs, live = _segment_buffers(pdtype, sdtype)
    before = [b.clone() for b in bufs]
    rows = [(b, e, lr, wd, step) for (b, e), (lr, wd, step) in zip(ranges, SEG_HP)]
    gl = _live_gradient(bufs, ranges)
    st = ops.grad_stats_flat(gl, grad_scale=0.5, max_norm=1.0)
    r = _rec(st)
    ref = R.clip_ref([gl.cpu()], 1.0, grad_scale=0.5)
    assert ref["clip_coef"] < 0.5 and R.within_f32_ulps(r["grad_mult"], ref["grad_mult"])
    _lib.check(_stats_step(bufs, rows, st, pdtype, sdtype), "sow_adamw_flat_seg_stats")
    torch.cuda.synchronize()
    _gaps_untouched(bufs, before, live, "clipped")
    _check_segments(bufs, before, ranges, SEG_HP, r["grad_mult"], pdtype, sdtype, "clipped")


@pytest.mark.parametrize("pdtype,sdtype", PAIRS, ids=PIDS)
def test_adamw_skips_a_non_finite_step_and_corrects_the_bias_on_the_device(pdtype, sdtype):
    hp = ((1e-2, 0.1, 1), (3e-4, 0.0, 1), (1e-3, 0.05, 1))
    ranges, bufs, live = _segment_buffers(pdtype, sdtype, hp=hp)
    before = [b.clone() for b in bufs]
    counters = torch.tensor([0, 3, 0, 9], dtype=torch.int32, device=DEV)       # segment k -> counter (2, 0, 3); 1 is unused
    idx = [2, 0, 3]
    gl = _live_gradient(bufs, ranges)
    bad = gl.clone()
    bad[517] = math.inf
    # (d) the same record without skip_nonfinite does step
    twin = [b.clone() for b in bufs]
    st = ops.grad_stats_flat(bad)                 # no clipping: grad_mult is 1 (with it, max_norm / inf = 0 and only decay acts)
    assert _rec(st)["nonfinite"] == 1 and _rec(st)["grad_mult"] == 1.0
    rows = [(b, e, lr, wd, 1) for (b, e), (lr, wd, _) in zip(ranges, hp)]
    _lib.check(_stats_step(twin, rows, st, pdtype, sdtype, skip=0), "sow_adamw_flat_seg_stats")
    assert not torch.equal(_bits(twin[0]), _bits(before[0]))
    # (c) skipped: nothing moves, every counter goes up by one
    st = ops.grad_stats_flat(bad, max_norm=1.0, skip_counters=counters)
    assert _rec(st)["nonfinite"] == 1
    _lib.check(_stats_step(bufs, rows, st, pdtype, sdtype, cnt_idx=idx, counters=counters, skip=1), "sow_adamw_flat_seg_stats")
    torch.cuda.synchronize()
    for nm, buf, old in zip("pgmv", bufs, before):
        assert torch.equal(_bits(buf), _bits(old)), f"{nm} moved on a skipped step"
    assert counters.cpu().tolist() == [1, 4, 1, 10]
    # the next, finite call: the host says step 2, the counters say one (segment 1: 1, others 1 and 10 -> max(1, 2 - c) = 1)
    st = ops.grad_stats_flat(gl, max_norm=1.0, skip_counters=counters)
    r = _rec(st)
    assert r["nonfinite"] == 0 and counters.cpu().tolist() == [1, 4, 1, 10]
    rows2 = [(b, e, lr, wd, 2) for (b, e), (lr, wd, _) in zip(ranges, hp)]
    _lib.check(_stats_step(bufs, rows2, st, pdtype, sdtype, cnt_idx=idx, counters=counters, skip=1), "sow_adamw_flat_seg_stats")
    torch.cuda.synchronize()
    _gaps_untouched(bufs, before, live, "after a skip")
    _check_segments(bufs, before, ranges, hp, r["grad_mult"], pdtype, sdtype, "after a skip", steps=[1, 1, 1])


def test_adamw_stats_refuses_a_bad_counter_index_and_writes_nothing():
    ranges, bufs, live = _segment_buffers(F32, F32)
    before = [b.clone() for b in bufs]
    rows = [(b, e, lr, wd, step) for (b, e), (lr, wd, step) in zip(ranges, SEG_HP)]
    st = ops.grad_stats_flat(_live_gradient(bufs, ranges))
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert _stats_step(bufs, rows, st, F32, F32, cnt_idx=[0, 1, 2], counters=counters, skip=1) == _lib.ERR_SHAPE
    assert _stats_step(bufs, rows, st, F32, F32, cnt_idx=[0, -2, 1], counters=counters, skip=1) == _lib.ERR_SHAPE
    torch.cuda.synchronize()
    for buf, old in zip(bufs, before):
        assert torch.equal(_bits(buf), _bits(old))


# ------------------------------------------------------------------------------------------------ 6. optimizer level
SHAPES = [(37, 5), (64,), (130, 3), (7,), (128, 2)]          # 185, 64, 390, 7, 256 elements: three of five slots are padded


def _bucket(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [nn.Parameter((torch.randn(s, generator=g) * 0.05).to(dtype).to(DEV)) for s in SHAPES]
    bucket = FactorBucket(ps)
    pad = torch.ones(bucket.padded_numel, dtype=torch.bool, device=DEV)
    for p, o in zip(ps, bucket.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 0
    return bucket, ps, pad


def _optimizer(bucket, ps, groups, sdtype=F32):
    pg = [{"params": ps[:3], "lr": 1e-2, "weight_decay": 0.1}, {"params": ps[3:], "lr": 3e-4, "weight_decay": 0.0}] if groups else None
    return FactorAdamW(bucket, lr=2e-3, weight_decay=0.05, state_dtype=sdtype, param_groups=pg)


def _fill_grads(ps, seed, scale, dtype):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad.copy_((torch.randn(p.shape, generator=g) * scale).to(dtype))


def _ranges_hp(opt, bucket, steps=None):
    """[(begin, end, lr, wd, step)] of the step the optimizer is about to take (steps: override per group)."""
    if opt._groups is None:
        return [(0, bucket.padded_numel, opt.lr, opt.weight_decay, (steps or [opt.step_count + 1])[0])]
    return [(b, e, opt._groups[gi]["lr"], opt._groups[gi]["weight_decay"], (steps or [s + 1 for s in opt.group_steps])[gi])
            for gi, b, e in opt._group_ranges()]


def _snapshot(bucket, opt):
    return [bucket.flat_param.clone(), bucket.flat_grad.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]


def _check_opt_step(bucket, opt, before, table, gm, name):
    pd, sd = bucket.flat_param.dtype, opt.exp_avg.dtype
    for b, e, lr, wd, step in table:
        p0, g0, m0, v0 = (t[b:e].cpu() for t in before)
        refs, mags = adamw_ref(p0, g0, m0, v0, lr=lr, betas=BETAS, eps=EPS, wd=wd, step=step, grad_scale=gm)
        out = dict(p=bucket.flat_param[b:e].cpu(), m=opt.exp_avg[b:e].cpu(), v=opt.exp_avg_sq[b:e].cpu())
        check_step(out, refs, mags, pd, sd, f"{name} [{b}, {e}) step {step}")


@pytest.mark.parametrize("groups", [False, True], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_optimizer_clipped_steps_against_fp64(dtype, groups):
    bucket, ps, pad = _bucket(dtype)
    opt = _optimizer(bucket, ps, groups)
    for k, scale in enumerate((1.0, 1e-3, 30.0)):                  # clipped, not clipped, clipped hard
        _fill_grads(ps, 10 + k, scale, dtype)
        before = _snapshot(bucket, opt)
        table = _ranges_hp(opt, bucket)
        st = opt.step(max_grad_norm=1.0)
        assert st is opt.last_grad_stats
        r = _rec(st)
        ref = R.clip_ref([p.grad.cpu() for p in ps], 1.0)
        assert abs(r["sumsq"] - ref["sumsq"]) <= R.sumsq_bound(bucket.padded_numel, ref["sumsq"])
        assert R.within_f32_ulps(r["total_norm"], ref["total_norm"]) and R.within_f32_ulps(r["grad_mult"], ref["grad_mult"])
        assert (r["clip_coef"] == 1.0) == (scale == 1e-3)
        _check_opt_step(bucket, opt, before, table, r["grad_mult"], f"step {k}")
        assert not bool(bucket.flat_grad[pad].any()) and not bool(bucket.flat_param[pad].any())
        assert torch.equal(_bits(bucket.flat_grad), _bits(before[1]))
    assert opt.step_count == 3 and opt._counters is None
    sd = opt.state_dict()
    assert sd["step"] == 3 and (not groups or sd["group_steps"] == [3, 3])
    # grad_scale = 0.5 halves the norm (a power of two: exactly)
    full, half = _rec(bucket.grad_stats()), _rec(bucket.grad_stats(grad_scale=0.5))
    assert half["total_norm"] == 0.5 * full["total_norm"] and half["sumsq"] == full["sumsq"]


@pytest.mark.parametrize("groups", [False, True], ids=["one-group", "two-groups"])
def test_optimizer_skipped_step_checkpoint_and_group_reset(groups):
    dtype = BF16
    bucket, ps, pad = _bucket(dtype, seed=1)
    opt = _optimizer(bucket, ps, groups)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True)
    _fill_grads(ps, 20, 1.0, dtype)
    opt.step(**kw)
    # a skipped step in the middle
    _fill_grads(ps, 21, 1.0, dtype)
    ps[2].grad.view(-1)[11] = math.inf
    before = _snapshot(bucket, opt)
    st = opt.step(**kw)
    assert _rec(st)["nonfinite"] == 1
    for a, b in zip(_snapshot(bucket, opt), before):
        assert torch.equal(_bits(a), _bits(b)), "a skipped step moved something"
    assert opt.step_count == 2 and opt.skip_counters.cpu().tolist() == [1] * (3 if groups else 1)
    # the step after it: host count 3, effective step 2 (bias correction formed on the device)
    _fill_grads(ps, 22, 1.0, dtype)
    before = _snapshot(bucket, opt)
    r = _rec(opt.step(**kw))
    _check_opt_step(bucket, opt, before, _ranges_hp(opt, bucket, steps=[2, 2]), r["grad_mult"], "after the skip")
    sd = opt.state_dict()
    assert sd["step"] == 2 and (not groups or sd["group_steps"] == [2, 2]), sd
    assert opt.skip_counters.cpu().tolist() == [0] * (3 if groups else 1) and opt.step_count == 2
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "lr", "betas", "eps", "weight_decay", "numel"} | (
        {"group_lr", "group_weight_decay", "group_steps"} if groups else set())
    # a fresh optimizer loaded from the checkpoint continues bit for bit with the original
    _fill_grads(ps, 23, 1.0, dtype)
    p_saved = bucket.flat_param.clone()
    opt.step(**kw)
    torch.cuda.synchronize()
    first = [bucket.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()]
    bucket.flat_param.copy_(p_saved)
    fresh = _optimizer(bucket, ps, groups)
    fresh.load_state_dict(sd)
    fresh.step(**kw)
    for nm, a, b in zip("pmv", first, [bucket.flat_param, fresh.exp_avg, fresh.exp_avg_sq]):
        assert torch.equal(_bits(a), _bits(b)), f"{nm}: the reloaded optimizer took another step"
    if not groups:
        return
    # reset_state(group) after a skip: that group is at step 1 on its next step, the other keeps its effective count
    _fill_grads(ps, 24, 1.0, dtype)
    ps[0].grad.view(-1)[3] = math.nan
    opt.step(**kw)                                        # skipped: host counts 4, counters 1
    opt.reset_state(0)
    assert opt.group_steps == [0, 4]
    _fill_grads(ps, 25, 1.0, dtype)
    before = _snapshot(bucket, opt)
    r = _rec(opt.step(**kw))
    assert r["nonfinite"] == 0
    _check_opt_step(bucket, opt, before, _ranges_hp(opt, bucket, steps=[1, 4]), r["grad_mult"], "after reset_state(0)")
    assert opt.skip_counters.cpu().tolist() == [0, 1, 1]
    sd = opt.state_dict()
    assert sd["group_steps"] == [1, 4] and sd["step"] == 4
    assert not bool(bucket.flat_grad[pad].any()) and not bool(bucket.flat_param[pad].any())


@pytest.mark.parametrize("groups", [False, True], ids=["one-group", "two-groups"])
def test_every_form_of_step_after_a_skip_uses_the_effective_step(groups):
    """The host counts hold a skipped step until state_dict() folds it: a clipping step without skip_nonfinite and a plain
    step() after it must read the counters too (first moments start at zero, so step 1 and step 2 differ by a factor 1.9)."""
    dtype = BF16
    bucket, ps, pad = _bucket(dtype, seed=5)
    opt = _optimizer(bucket, ps, groups)
    _fill_grads(ps, 60, 1.0, dtype)
    ps[1].grad.view(-1)[2] = math.inf
    assert _rec(opt.step(max_grad_norm=1.0, skip_nonfinite=True))["nonfinite"] == 1          # host count 1, effective 0
    for k, kw in enumerate((dict(max_grad_norm=1.0), dict())):
        _fill_grads(ps, 61 + k, 1.0, dtype)
        before = _snapshot(bucket, opt)
        r = _rec(opt.step(0.5, **kw))
        assert r["nonfinite"] == 0 and (r["clip_coef"] == 1.0) == (not kw) and (kw or r["grad_mult"] == 0.5)
        _check_opt_step(bucket, opt, before, _ranges_hp(opt, bucket, steps=[k + 1, k + 1]), r["grad_mult"], f"form {k} after a skip")
    sd = opt.state_dict()
    assert sd["step"] == 2 and (not groups or sd["group_steps"] == [2, 2])


def test_step_with_defaults_is_the_plain_step():
    """No new keyword, nothing armed: the same bits as the C calls the method has always made, and no record."""
    for groups in (False, True):
        outs = []
        for which in range(2):
            bucket, ps, _ = _bucket(BF16, seed=2)
            opt = _optimizer(bucket, ps, groups)
            _fill_grads(ps, 30, 1.0, BF16)
            if which == 0:
                assert opt.step(0.5) is None and opt.last_grad_stats is None and opt._counters is None
            elif groups:
                ops.adamw_flat_seg_(bucket.flat_param, bucket.flat_grad, opt.exp_avg, opt.exp_avg_sq, opt.segments(),
                                    betas=opt.betas, eps=opt.eps, grad_scale=0.5)
            else:
                ops.adamw_flat_(bucket.flat_param, bucket.flat_grad, opt.exp_avg, opt.exp_avg_sq, lr=opt.lr, betas=opt.betas,
                                eps=opt.eps, weight_decay=opt.weight_decay, step=1, grad_scale=0.5)
            outs.append([bucket.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()])
        for a, b in zip(*outs):
            assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 7. clip_grad_norm_
def test_clip_grad_norm_over_bucket_and_dense_parameters():
    dtype = BF16
    bucket, ps, pad = _bucket(dtype, seed=3)
    opt = _optimizer(bucket, ps, groups=True)
    g = torch.Generator().manual_seed(40)
    dense = [nn.Parameter(torch.randn(33, 9, generator=g).to(DEV)), nn.Parameter(torch.randn(70, generator=g).to(DEV))]
    for d in dense:
        d.grad = (torch.randn(d.shape, generator=g) * 2.0).to(DEV)
    unused = nn.Parameter(torch.zeros(3, device=DEV))               # no gradient: skipped, as torch does
    _fill_grads(ps, 41, 1.0, dtype)
    dense0 = [d.grad.clone() for d in dense]
    flat0 = bucket.flat_grad.clone()
    before = _snapshot(bucket, opt)
    total = clip_grad_norm_(opt, dense + [unused], 1.0)
    assert total.is_cuda and total.dim() == 0 and total.dtype == F32
    st = opt._armed_stats
    r = _rec(st)
    extra = R.sumsq([d.cpu() for d in dense0])
    ref = R.clip_ref([p.grad.cpu() for p in ps], 1.0, extra_sq=extra)
    allref = R.clip_ref([p.grad.cpu() for p in ps] + [d.cpu() for d in dense0], 1.0)
    assert abs(allref["total_norm"] - ref["total_norm"]) <= 2.0 ** -50 * ref["total_norm"]
    assert R.within_f32_ulps(float(total), allref["total_norm"])
    assert R.within_f32_ulps(r["clip_coef"], ref["clip_coef"]) and r["clip_coef"] < 0.2
    assert R.within_f32_ulps(r["grad_mult"], ref["grad_mult"])
    coef = torch.tensor(r["clip_coef"], dtype=F32)
    for d, d0 in zip(dense, dense0):
        assert torch.equal(d.grad.cpu(), d0.cpu() * coef), "the dense gradients are scaled by the record's coefficient"
    assert torch.equal(_bits(bucket.flat_grad), _bits(flat0)), "clip_grad_norm_ must not touch flat_grad"
    table = _ranges_hp(opt, bucket)
    assert opt.step() is st and opt._armed_stats is None
    _check_opt_step(bucket, opt, before, table, r["grad_mult"], "armed step")
    # the step after that, without re-arming, is an ordinary unclipped one
    before = _snapshot(bucket, opt)
    table = _ranges_hp(opt, bucket)
    assert opt.step() is None
    _check_opt_step(bucket, opt, before, table, 1.0, "unarmed step")
    # an armed record that says "overflow" makes a skipping step leave everything alone, and the step is counted as skipped
    before = _snapshot(bucket, opt)
    clip_grad_norm_(opt, dense, 1.0, found_inf=torch.ones(1, device=DEV))
    assert _rec(opt.step(skip_nonfinite=True))["nonfinite"] == 1
    for a, b in zip(_snapshot(bucket, opt), before):
        assert torch.equal(_bits(a), _bits(b))
    assert opt.skip_counters.cpu().tolist() == [1, 1, 1] and opt.state_dict()["group_steps"] == [2, 2]
    # arming with one grad_scale and stepping with another is refused
    clip_grad_norm_(opt, dense, 1.0, grad_scale=0.5)
    with pytest.raises(ValueError, match="grad_scale"):
        opt.step(grad_scale=0.25)


# ------------------------------------------------------------------------------------------------ 8. capture
def test_whole_step_in_one_hip_graph():
    """grad_stats + AdamW captured once (a linear chain on one stream: nothing on the path may synchronise or allocate) and
    replayed on a small-norm fill, a large-norm fill and one with an inf; each replay equals the eager call bit for bit."""
    dtype = BF16
    bucket, ps, pad = _bucket(dtype, seed=4)
    opt = _optimizer(bucket, ps, groups=True)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True)
    _fill_grads(ps, 50, 1.0, dtype)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step(**kw)                                    # warm-up: creates the counters, the record and the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    state0 = [bucket.flat_param.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.skip_counters.clone()]
    host0 = (opt.step_count, list(opt.group_steps))

    def restore():
        for dst, src in zip((bucket.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.skip_counters), state0):
            dst.copy_(src)
        opt.step_count, opt.group_steps = host0[0], list(host0[1])

    def result(st):
        torch.cuda.synchronize()
        return [_bits(bucket.flat_param).clone(), _bits(opt.exp_avg.to(F32)).clone(), _bits(opt.exp_avg_sq.to(F32)).clone(),
                opt.skip_counters.clone(), st.buf.clone()]

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st_graph = opt.step(**kw)
    fills = {"small": (51, 1e-3, None), "large": (52, 30.0, None), "inf": (53, 1.0, math.inf)}
    for name, (seed, scale, poison) in fills.items():
        _fill_grads(ps, seed, scale, dtype)
        if poison is not None:
            ps[1].grad.view(-1)[5] = poison
        restore()
        graph.replay()
        replayed = result(st_graph)
        restore()
        eager = result(opt.step(**kw))
        for i, (a, b) in enumerate(zip(replayed, eager)):
            assert torch.equal(a, b), f"{name}: replay and eager differ in item {i}"
        rec = dict(zip(("sumsq", "total_sq", "total_norm", "clip_coef", "grad_mult", "nonfinite"),
                       struct.unpack("<ddfffi", bytes(replayed[4].cpu().numpy().tobytes()))))
        if name == "inf":
            assert rec["nonfinite"] == 1 and torch.equal(replayed[0], _bits(state0[0])), "the inf replay moved the parameters"
            assert torch.equal(replayed[1], _bits(state0[1].to(F32))) and torch.equal(replayed[2], _bits(state0[2].to(F32)))
            assert replayed[3].cpu().tolist() == (state0[3] + 1).cpu().tolist()
        else:
            assert rec["nonfinite"] == 0 and (rec["clip_coef"] == 1.0) == (name == "small")
            assert not torch.equal(replayed[0], _bits(state0[0]))


# ------------------------------------------------------------------------------------------------ 9. training-step padding
class _Block(nn.Module):
    """The llama-shaped block of tests/test_gpu_autocast.py, with widths and a rank that leave every factor slot of the
    bucket padded (264 * 10 and 520 * 10 are no multiples of 64)."""

    def __init__(self, d=264, dff=520, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        mk = lambda i, o: SoWLinear(i, o, bias=False, rank=10, init_method="normal", device=DEV)
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = mk(d, d), mk(d, d), mk(d, d), mk(d, d)
        self.gate_proj, self.up_proj, self.down_proj = mk(d, dff), mk(d, dff), mk(dff, d)

    def forward(self, h):
        a = self.q_proj(h) * self.k_proj(h) + self.v_proj(h)
        h = h + self.o_proj(a)
        return h + self.down_proj(F.silu(self.gate_proj(h)) * self.up_proj(h))


def test_training_step_leaves_the_padding_zero():
    net = nn.Sequential(_Block(seed=1), _Block(seed=2))
    bucket = FactorBucket(factor_parameters(net))
    assert bucket.attach(net) == 14
    pad = torch.ones(bucket.padded_numel, dtype=torch.bool, device=DEV)
    for p, o in zip(bucket.params, bucket.offsets):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) >= 28 * 16
    x = torch.randn(2, 512, 264, device=DEV)
    bucket.zero_grad()
    with torch.autocast("cuda", dtype=BF16):
        y = net(x)
    y.float().square().mean().backward()
    st = bucket.grad_stats()                              # finalize() is its first act
    assert not bool(bucket.flat_grad[pad].any()), "a kernel wrote into the padding of flat_grad"
    ref = R.sumsq([p.grad.cpu() for p in bucket.params])
    r = _rec(st)
    assert ref > 0 and abs(r["sumsq"] - ref) <= R.sumsq_bound(bucket.padded_numel, ref), (r["sumsq"], ref)
