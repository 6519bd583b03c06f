"""sow_adamw_flat_seg (AdamW over segments of one flat buffer, each with its own lr, weight decay and step) at the C ABI:
bit-identity with sow_adamw_flat on one segment, element-wise fp64 checks per segment (tests/step_numerics.py), untouched
gaps and guards in all four buffers, error codes, and a table longer than one launch takes."""
import ctypes

import pytest
import torch

from step_numerics import adamw_ref, check_step
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: _lib.F32, BF16: _lib.BF16, F16: _lib.F16}
INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]
IDS = ["f32-f32", "bf16-bf16", "bf16-f32", "f16-f16", "f16-f32"]
GUARD = 64
BETAS, EPS = (0.9, 0.999), 1e-8


def _bits(t):
    return t.view(INT[t.dtype])


def _s():
    return torch.cuda.current_stream().cuda_stream


def _segs(rows):
    return (_lib.AdamwSegment * max(len(rows), 1))(*[_lib.AdamwSegment(*r) for r in rows]), len(rows)


def _data(n, pdtype, sdtype, seed):
    """p, g, m, v on the CPU: zero, tiny and large gradients, a resumed state."""
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
    """Distinct NaN bit patterns (quiet NaNs with a running payload), so that a copied or rewritten NaN shows."""
    n = t.numel()
    if t.dtype == F32:
        _bits(t).copy_((0x7FC00001 + torch.arange(n, device=t.device) % 4096).to(torch.int32))
    else:
        base = 0x7FC1 if t.dtype == BF16 else 0x7E01
        _bits(t).copy_((base + torch.arange(n, device=t.device) % 32).to(torch.int16))
    return t


def _seg_call(lib, p, g, m, v, rows, pdtype, sdtype, gs=1.0):
    arr, n = _segs(rows)
    return lib.sow_adamw_flat_seg(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), arr, n, BETAS[0], BETAS[1], EPS, gs,
                                  DT[pdtype], DT[sdtype], _s())


def _flat_call(lib, p, g, m, v, n, lr, wd, step, pdtype, sdtype, gs=1.0):
    return lib.sow_adamw_flat(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, BETAS[0], BETAS[1], EPS, wd, step,
                              gs, DT[pdtype], DT[sdtype], _s())


@pytest.mark.parametrize("pdtype,sdtype", PAIRS, ids=IDS)
@pytest.mark.parametrize("n", [64 * 5 + 192, 1, 63, 65])
def test_one_segment_equals_adamw_flat_bit_for_bit(pdtype, sdtype, n):
    lib = _lib.load()
    p0, g0, m0, v0 = _data(n, pdtype, sdtype, seed=n)
    outs = []
    for which in ("flat", "seg"):
        # the unpadded C call: n elements with NaN guards on both sides
        bufs = [_nan_fill(torch.empty(n + 2 * GUARD, dtype=t.dtype, device=DEV)) for t in (p0, g0, m0, v0)]
        before = [_bits(b).clone() for b in bufs]
        views = [b[GUARD:GUARD + n] for b in bufs]
        for vw, t in zip(views, (p0, g0, m0, v0)):
            vw.copy_(t)
        p, g, m, v = views
        if which == "flat":
            _lib.check(_flat_call(lib, p, g, m, v, n, 3e-3, 0.1, 7, pdtype, sdtype, gs=0.5), "sow_adamw_flat")
        else:
            _lib.check(_seg_call(lib, p, g, m, v, [(0, n, 3e-3, 0.1, 7)], pdtype, sdtype, gs=0.5), "sow_adamw_flat_seg")
        torch.cuda.synchronize()
        for b, b0 in zip(bufs, before):
            assert torch.equal(_bits(b)[:GUARD], b0[:GUARD]) and torch.equal(_bits(b)[GUARD + n:], b0[GUARD + n:]), which
        assert torch.equal(_bits(g), _bits(g0.to(DEV)))
        outs.append([_bits(t).clone() for t in (p, m, v)])
    for name, a, b in zip("pmv", *outs):
        assert torch.equal(a, b), f"{name}: one segment [0, {n}) differs from sow_adamw_flat"
    assert not torch.equal(outs[0][0], _bits(p0.to(DEV)))      # the step did move the parameters


# guard | segment 0 | segment 1 | gap | segment 2 | guard: odd lengths, more than one workgroup each, misaligned starts
SEG_LEN = (300, 1000, 777)
SEG_HP = ((1e-2, 0.1, 1), (3e-4, 0.0, 7), (1e-3, 0.05, 1000))      # lr, weight decay, step


@pytest.mark.parametrize("pdtype,sdtype", PAIRS, ids=IDS)
def test_three_segments_against_fp64_and_untouched_gaps(pdtype, sdtype):
    lib = _lib.load()
    b0 = GUARD
    b1 = b0 + SEG_LEN[0]
    b2 = b1 + SEG_LEN[1] + 64
    total = b2 + SEG_LEN[2] + GUARD
    ranges = [(b0, b1), (b1, b1 + SEG_LEN[1]), (b2, b2 + SEG_LEN[2])]
    host = _data(total, pdtype, sdtype, seed=3)
    bufs = [_nan_fill(torch.empty(total, dtype=t.dtype, device=DEV)) for t in host]
    live = torch.zeros(total, dtype=torch.bool, device=DEV)
    for (b, e), (_, _, step) in zip(ranges, SEG_HP):
        live[b:e] = True
        for buf, t in zip(bufs, host):
            buf[b:e].copy_(t[b:e])
        if step == 1:                                      # a first step starts from zero moments
            bufs[2][b:e].zero_()
            bufs[3][b:e].zero_()
    before = [b.clone() for b in bufs]
    rows = [(b, e, lr, wd, step) for (b, e), (lr, wd, step) in zip(ranges, SEG_HP)]
    _lib.check(_seg_call(lib, *bufs, rows, pdtype, sdtype, gs=0.5), "sow_adamw_flat_seg")
    torch.cuda.synchronize()
    for name, buf, old in zip(("p", "g", "m", "v"), bufs, before):
        same = _bits(buf) == _bits(old)
        assert bool(same[~live].all()), f"{name}: {int((~same[~live]).sum())} elements outside every segment were rewritten"
    assert torch.equal(_bits(bufs[1]), _bits(before[1]))   # the gradient is read only
    for k, ((b, e), (lr, wd, step)) in enumerate(zip(ranges, SEG_HP)):
        p0, g0, m0, v0 = (t[b:e].cpu() for t in before)
        refs, mags = adamw_ref(p0, g0, m0, v0, lr=lr, betas=BETAS, eps=EPS, wd=wd, step=step, grad_scale=0.5)
        out = dict(p=bufs[0][b:e].cpu(), m=bufs[2][b:e].cpu(), v=bufs[3][b:e].cpu())
        stats = check_step(out, refs, mags, pdtype, sdtype, f"segment {k} (lr {lr}, wd {wd}, step {step})")
        print(f"segment {k} {pdtype}/{sdtype}: " + ", ".join(f"{q} {s['worst']:.3g}" for q, s in stats.items()))


def test_error_codes_and_nothing_written():
    lib = _lib.load()
    n = 512
    host = _data(n, F32, F32, seed=5)
    bufs = [t.to(DEV) for t in host]
    before = [b.clone() for b in bufs]
    good = (0, 100, 1e-3, 0.0, 1)
    bad = {
        "overlapping": [good, (99, 200, 1e-3, 0.0, 1)],
        "unsorted": [(200, 300, 1e-3, 0.0, 1), good],
        "step 0": [good, (100, 200, 1e-3, 0.0, 0)],
        "empty": [good, (100, 100, 1e-3, 0.0, 1)],
        "reversed": [good, (200, 150, 1e-3, 0.0, 1)],
        "negative": [(-4, 100, 1e-3, 0.0, 1)],
    }
    for what, rows in bad.items():
        assert _seg_call(lib, *bufs, rows, F32, F32) == _lib.ERR_SHAPE, what
    arr, k = _segs([good])
    args = (BETAS[0], BETAS[1], EPS, 1.0, _lib.F32, _lib.F32, _s())
    ptrs = [b.data_ptr() for b in bufs]
    for i in range(4):
        q = list(ptrs)
        q[i] = None
        assert lib.sow_adamw_flat_seg(*q, arr, k, *args) == _lib.ERR_NULL, i
    assert lib.sow_adamw_flat_seg(*ptrs, None, 1, *args) == _lib.ERR_NULL
    assert lib.sow_adamw_flat_seg(*ptrs, arr, -1, *args) == _lib.ERR_SHAPE
    assert lib.sow_adamw_flat_seg(*ptrs, arr, 0, *args) == 0
    assert lib.sow_adamw_flat_seg(*ptrs, arr, 1, BETAS[0], BETAS[1], EPS, 1.0, _lib.F32, _lib.BF16, _s()) == -3   # SOW_ERR_DTYPE
    torch.cuda.synchronize()
    for b, old in zip(bufs, before):
        assert torch.equal(_bits(b), _bits(old))          # a refused table launches nothing, not even its good segments
    # touching segments are not overlapping
    assert _seg_call(lib, *bufs, [good, (100, 200, 1e-3, 0.0, 2)], F32, F32) == 0


@pytest.mark.parametrize("pdtype,sdtype", [(F32, F32), (BF16, F32)], ids=["f32-f32", "bf16-f32"])
def test_more_segments_than_one_launch_takes(pdtype, sdtype):
    """Twice the per-launch cap of 2-element segments, one untouched element between neighbours, every segment with its
    own lr, weight decay and step: equal, bit for bit, to one sow_adamw_flat call per segment."""
    lib = _lib.load()
    nseg = 2 * _lib.ADAMW_MAX_SEGMENTS
    total = 3 * nseg + 1
    host = _data(total, pdtype, sdtype, seed=11)
    rows = [(3 * i + 1, 3 * i + 3, 1e-3 * (1 + i % 7), 0.01 * (i % 3), 1 + 13 * i) for i in range(nseg)]
    seg = [t.to(DEV) for t in host]
    ref = [t.to(DEV) for t in host]
    _lib.check(_seg_call(lib, *seg, rows, pdtype, sdtype, gs=2.0), "sow_adamw_flat_seg")
    for b, e, lr, wd, step in rows:
        _lib.check(_flat_call(lib, *[t[b:e] for t in ref], e - b, lr, wd, step, pdtype, sdtype, gs=2.0), "sow_adamw_flat")
    torch.cuda.synchronize()
    for name, a, b, t0 in zip(("p", "g", "m", "v"), seg, ref, host):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: differs from per-segment sow_adamw_flat calls"
        assert torch.equal(_bits(a)[0::3], _bits(t0.to(DEV))[0::3]), f"{name}: an element between two segments was rewritten"
    assert not torch.equal(_bits(seg[0])[1::3], _bits(host[0].to(DEV))[1::3])
    assert not torch.equal(_bits(seg[0])[3 * nseg - 1], _bits(host[0].to(DEV))[3 * nseg - 1])   # the second launch ran too
