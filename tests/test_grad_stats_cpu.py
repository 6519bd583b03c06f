"""Host side of the device gradient record (sow_grad_stats_flat, sow_adamw_flat_seg_stats, FactorAdamW.step's clipping
keywords, sow_amd.clip_grad_norm_): exports, the workspace query, every validation error (all of them return before the
first HIP call, so no GPU is needed), the float64 reference of the GPU tests against torch, and the refusals on a CPU bucket."""
import ctypes
import math

import pytest
import torch

import grad_stats_ref as R
from sow_amd import _lib

NAMES = ("sow_grad_stats_workspace_bytes", "sow_grad_stats_flat", "sow_adamw_flat_seg_stats")
FAKE = 0x10000      # a non-null "device pointer": the refused calls never dereference it


def test_library_exports_the_three_symbols():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert ctypes.sizeof(_lib.GradStatsRecord) == 32
    assert [f[0] for f in _lib.GradStatsRecord._fields_] == ["sumsq", "total_sq", "total_norm", "clip_coef", "grad_mult",
                                                             "nonfinite"]
    assert _lib.GradStatsRecord.total_norm.offset == 16 and _lib.GradStatsRecord.nonfinite.offset == 28


def test_workspace_query_is_zero_safe_and_monotone():
    lib = _lib.load()
    q = lib.sow_grad_stats_workspace_bytes
    assert q(0) >= 8 and q(-5) == q(0)
    ns = [0, 1, 7, 2047, 2048, 2049, 4096, 4097, 2048 * 1023, 2048 * 1024, 2048 * 1024 + 1, 2048 * 1025, 3 * 2 ** 20 + 5,
          2 ** 31 + 9, 2 ** 40]
    sizes = [q(n) for n in ns]
    assert sizes == sorted(sizes), sizes
    assert q(2048) == 8 and q(2049) == 16 and max(sizes) == 8 * 1024


def _stats_call(lib, grad=FAKE, n=100, dtype=_lib.F32, counters=None, n_counters=0, ws=FAKE, ws_bytes=8192, out=FAKE):
    return lib.sow_grad_stats_flat(grad, n, dtype, 1.0, 1.0, None, None, None, counters, n_counters, ws, ws_bytes, out, None)


def test_grad_stats_validation_errors():
    lib = _lib.load()
    assert _stats_call(lib, n=-1) == _lib.ERR_SHAPE
    assert _stats_call(lib, n_counters=-1) == _lib.ERR_SHAPE
    assert _stats_call(lib, grad=None) == _lib.ERR_NULL
    assert _stats_call(lib, out=None) == _lib.ERR_NULL
    assert _stats_call(lib, ws=None) == _lib.ERR_NULL
    assert _stats_call(lib, grad=None, n=0, out=None) == _lib.ERR_NULL           # n == 0 admits a null grad, not a null out
    assert _stats_call(lib, counters=None, n_counters=2) == _lib.ERR_NULL
    assert _stats_call(lib, dtype=7) == _lib.ERR_DTYPE
    assert _stats_call(lib, dtype=_lib.BF16 | _lib.PARAM_F32) == _lib.ERR_DTYPE
    for n in (1, 2049, 2048 * 1024 + 8):
        need = lib.sow_grad_stats_workspace_bytes(n)
        assert _stats_call(lib, n=n, ws_bytes=need - 1) == _lib.ERR_WORKSPACE, n
    assert _stats_call(lib, n=0, grad=None, ws_bytes=7) == _lib.ERR_WORKSPACE


def _seg_call(lib, rows, counters=None, n_segs=None, p=FAKE, g=FAKE, m=FAKE, v=FAKE, stats=FAKE, skip=None, n_counters=0,
              dtype=_lib.F32, sdtype=_lib.F32, null_segs=False):
    arr = (_lib.AdamwSegment * max(len(rows), 1))(*[_lib.AdamwSegment(*r) for r in rows])
    cnt = None if counters is None else (ctypes.c_int * max(len(counters), 1))(*counters)
    return lib.sow_adamw_flat_seg_stats(p, g, m, v, None if null_segs else arr, cnt, len(rows) if n_segs is None else n_segs,
                                        0.9, 0.999, 1e-8, stats, 1, skip, n_counters, dtype, sdtype, None)


def test_adamw_stats_validation_errors():
    lib = _lib.load()
    good = (0, 100, 1e-3, 0.0, 1)
    for k in ("p", "g", "m", "v", "stats"):
        assert _seg_call(lib, [good], **{k: None}) == _lib.ERR_NULL, k
    assert _seg_call(lib, [good], null_segs=True) == _lib.ERR_NULL
    assert _seg_call(lib, [good], counters=[0], n_counters=1, skip=None) == _lib.ERR_NULL
    assert _seg_call(lib, [good], n_segs=-1) == _lib.ERR_SHAPE
    assert _seg_call(lib, [good], n_counters=-1) == _lib.ERR_SHAPE
    bad = {
        "overlapping": [good, (99, 200, 1e-3, 0.0, 1)],
        "unsorted": [(200, 300, 1e-3, 0.0, 1), good],
        "step 0": [good, (100, 200, 1e-3, 0.0, 0)],
        "empty": [good, (100, 100, 1e-3, 0.0, 1)],
        "negative": [(-4, 100, 1e-3, 0.0, 1)],
    }
    for what, rows in bad.items():
        assert _seg_call(lib, rows) == _lib.ERR_SHAPE, what
    for cnt in ([2], [-2], [0]):
        nc = 2 if cnt != [0] else 0
        assert _seg_call(lib, [good], counters=cnt, n_counters=nc, skip=FAKE if nc else None) == _lib.ERR_SHAPE, cnt
    assert _seg_call(lib, [good], sdtype=_lib.BF16) == _lib.ERR_DTYPE
    assert _seg_call(lib, [good], dtype=_lib.F16, sdtype=_lib.BF16) == _lib.ERR_DTYPE
    assert _seg_call(lib, [], n_segs=0) == 0              # an empty table launches nothing


def test_reference_agrees_with_torch_clip_grad_norm():
    g = torch.Generator().manual_seed(0)
    shapes = [(7, 5), (33,), (4, 4, 3)]
    base = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    true_norm = math.sqrt(sum(float(t.square().sum()) for t in base))
    for max_norm in (true_norm * 2.0, true_norm / 3.0, math.inf):           # norm < max, norm > max, max = inf
        params = [torch.nn.Parameter(torch.zeros_like(t)) for t in base]
        for p, t in zip(params, base):
            p.grad = t.clone()
        got = torch.nn.utils.clip_grad_norm_(params, max_norm)
        ref = R.clip_ref(base, max_norm)
        assert abs(float(got) - ref["total_norm"]) <= 4 * 2.0 ** -52 * ref["total_norm"]
        if max_norm > true_norm:
            assert ref["clip_coef"] == 1.0
        else:
            assert ref["clip_coef"] < 1.0
        for p, t in zip(params, base):
            want = t * ref["clip_coef"]
            assert torch.allclose(p.grad, want, rtol=4 * 2.0 ** -52, atol=0.0)
    # the scales: grad_scale / loss_scale multiplies the norm, extra_sq adds under the root
    r = R.record(4.0, grad_scale=0.5, loss_scale=4.0, max_norm=0.125, extra_sq=0.0625 * 3)
    assert r["total_sq"] == 0.25 and r["total_norm"] == 0.5
    assert r["clip_coef"] == 0.125 / (0.5 + 1e-6) and r["grad_mult"] == 0.125 * r["clip_coef"] and r["nonfinite"] == 0
    assert R.record(math.inf)["nonfinite"] == 1 and R.record(1.0, found_inf=1.0)["nonfinite"] == 1
    assert R.record(math.inf, max_norm=1.0)["clip_coef"] == 1.0


def test_one_fp32_ulp_is_the_spacing_at_the_value():
    import numpy as np
    for x in (1.0, 1.5, 1.9999999, 2.0, 0.7, 3e-3, 123456.789, 2.0 ** -126, 2.0 ** -130, 3e38):
        assert R.f32_ulp(x) == float(np.spacing(np.float32(x))) == R.f32_ulp(-x), x
    below = 2.0 - 2.0 ** -23                                  # the last fp32 below 2: the spacing there is 2^-23, not 2^-22
    assert R.within_f32_ulps(below - 2.0 ** -23, below) and R.within_f32_ulps(2.0, below)
    assert not R.within_f32_ulps(below - 1.5 * 2.0 ** -23, below)     # 2^-23 |want| would have let this pass
    assert R.within_f32_ulps(0.0, 0.0) and not R.within_f32_ulps(1e-45, 0.0)


def _cpu_optimizer(groups=False):
    from sow_amd import FactorAdamW, FactorBucket
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(70))]
    bucket = FactorBucket(ps)
    pg = [{"params": [ps[0]]}, {"params": [ps[1]], "weight_decay": 0.0}] if groups else None
    return FactorAdamW(bucket, lr=1e-3, param_groups=pg), bucket, ps


@pytest.mark.parametrize("groups", [False, True])
def test_cpu_bucket_has_no_fallback(groups):
    import sow_amd
    opt, bucket, ps = _cpu_optimizer(groups)
    before = bucket.flat_param.clone()
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(loss_scale=2.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bucket.grad_stats(max_norm=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sow_amd.clip_grad_norm_(opt, [], 1.0)
    assert torch.equal(bucket.flat_param, before) and opt.step_count == 0 and opt.last_grad_stats is None


@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0), dict(loss_scale=2.0), dict(extra_sq_norm=0.0),
                                dict(found_inf=torch.zeros(1))], ids=lambda kw: next(iter(kw)))
def test_step_with_a_record_refuses_the_keywords_the_record_already_holds(kw):
    from sow_amd import ops
    opt, bucket, _ = _cpu_optimizer()
    rec = ops.GradStats(torch.zeros(32, dtype=torch.uint8), grad_scale=0.5)
    opt.arm_grad_stats(rec)
    with pytest.raises(ValueError, match=next(iter(kw))):
        opt.step(**kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        opt.step(stats=rec, **kw)
    with pytest.raises(ValueError, match="grad_scale"):
        opt.step(grad_scale=0.25, stats=rec)
    assert opt.step_count == 0


def test_armed_step_refuses_another_grad_scale():
    from sow_amd import ops
    opt, bucket, _ = _cpu_optimizer()
    opt.arm_grad_stats(ops.GradStats(torch.zeros(32, dtype=torch.uint8), grad_scale=0.5))
    with pytest.raises(ValueError, match="grad_scale"):
        opt.step(grad_scale=0.25)
    # the record was consumed by the refused call: the next step is an ordinary one again (and, on a CPU bucket, refused as such)
    assert opt._armed_stats is None
    with pytest.raises(ValueError, match="32 contiguous bytes"):
        ops.GradStats(torch.zeros(16, dtype=torch.uint8))
    assert opt.state_dict()["step"] == 0
