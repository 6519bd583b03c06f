"""-m gpu: the module surface of the 33 ... 64-row skinny forward: inside sow_amd.skinny_rows(n), no-grad SoWLinear and
SiblingGroup calls of 33 ... n flattened rows take sow_forward_skinny_rows (quantised layers on their codes, no image); outside
it, and for everything the entry does not admit, today's path -- whose bits at T = 64 existing tests pin to the training forward."""
import pytest
import torch
import torch.nn as nn

import sow_amd
import test_gpu_acc_native as N
import test_gpu_elementwise as E
import test_gpu_fp8_acc as F8
import test_gpu_skinny as S
import test_gpu_skinny_rows as R
from numerics import bound, check_bound, fp32_floor, rne, to64
from sow_amd import _lib, ops, quantize_accumulators

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PATTERN = [3, 1, 2, 1, 3, 1, 2, 1]      # per block: q / k / v in one call, o, gate / up in one call, down
FMT_OF = {torch.float8_e4m3fn: "fp8", torch.uint8: "fp4"}


def _count(monkeypatch):
    """(calls of ops.sow_forward_skinny_rows, calls of ops.sow_forward_skinny), counted as test_gpu_skinny._count_skinny does."""
    rows, old = [], S._count_skinny(monkeypatch)
    orig = ops.sow_forward_skinny_rows
    monkeypatch.setattr(ops, "sow_forward_skinny_rows", lambda layers: (rows.append(len(layers)), orig(layers))[1])
    return rows, old


def _cabi(m, xin, flagged=False):
    """The C-ABI result of one projection from the module's own tensors, through sow_forward_skinny_rows."""
    acc_down, acc_up = m._acc_pair()
    d = dict(x=xin.reshape(-1, xin.shape[-1]).cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(),
             bias=None if m.bias is None else m.bias.data.cpu(), s=float(m.scale))
    if acc_down is None or acc_down.numel() == 0:
        d["fmt"] = "none"
    elif acc_down.dtype in FMT_OF:
        d.update(fmt=FMT_OF[acc_down.dtype], q=acc_down.data.view(torch.uint8).cpu(), e=acc_up.cpu())
    else:
        d.update(fmt="dense", W=acc_down.data.cpu())
    (y,) = R._run(xin.dtype, [d], runs=(0xFF,), flagged=flagged, what="module projection")
    return y


def _layer(d_in, d_out, r, dtype, acc="dense", seed=3):
    g = torch.Generator().manual_seed(seed)
    m = sow_amd.SoWLinear(d_in, d_out, bias=True, rank=r, init_method="normal", scale=0.5, device=DEV, dtype=dtype)
    with torch.no_grad():
        m.upscale_weights[0].copy_((torch.randn(r, d_out, generator=g) * 0.05).to(dtype))
        m.bias.copy_((torch.randn(d_out, generator=g) * 0.1).to(dtype))
    if acc == "dense":
        m.acc_downweight = nn.Parameter((torch.randn(d_in, d_out, generator=g) * 0.02).to(DEV, dtype), requires_grad=False)
    elif acc == "lowrank":
        m.acc_downweight = nn.Parameter((torch.randn(d_in, 16, generator=g) * 0.1).to(DEV, dtype), requires_grad=False)
        m.acc_upweight = nn.Parameter((torch.randn(16, d_out, generator=g) * 0.1).to(DEV, dtype), requires_grad=False)
    return m


def _image(m):
    """The accumulator of a layer as the reference sees it: the tensor itself, or the image W^ of its codes."""
    if not m.acc_quantized():
        return m.acc_downweight.data
    (img, _), = ops.acc_operands([m._acc_pair()], m.downscale_weights[0].dtype)
    return img.clone()


def _clear_qkv_ties(net, x):
    """q / k / v of the first block are the projections held to float64 here (their input is x itself): their h = s x A is moved
    clear of rounding ties first (skinny_sweep.off_ties, decided on the CPU from the operands alone, as in
    test_gpu_skinny_rows.py; DESIGN 4.5b has the reason).  Returns the three layers."""
    qkv = list(net.layers[0].self_attn.children())[:3]
    for m in qkv:
        d0 = dict(x=x.reshape(-1, x.shape[-1]).cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(), bias=None,
                  W=_image(m).cpu(), s=float(m.scale))
        with torch.no_grad():
            m.downscale_weights[0].copy_(R.SW.off_ties(x.dtype, d0)[0]["A"])
    return qkv


def test_the_setting():
    assert ops.skinny_rows_limit() == 32 and ops.SKINNY_MAX_T == 32
    with sow_amd.skinny_rows(64):
        assert ops.skinny_rows_limit() == 64
        with sow_amd.skinny_rows(48):
            assert ops.skinny_rows_limit() == 48
        assert ops.skinny_rows_limit() == 64
    assert ops.skinny_rows_limit() == 32
    for bad in (65, 31, 0, -1, 48.0, True, None):
        with pytest.raises(ValueError):
            sow_amd.set_skinny_rows(bad)
        with pytest.raises(ValueError):
            with sow_amd.skinny_rows(bad):
                pass
    assert ops.skinny_rows_limit() == 32
    assert sow_amd.set_skinny_rows(40) == 32 and sow_amd.set_skinny_rows(32) == 40
    for f in (ops.skinny_rows_pays, *(fmt.pays_rows for fmt in ops.FORMATS.values())):
        assert f(33, 4096, 4096) and f(64, 4096, 4096) and not f(32, 4096, 4096) and not f(65, 4096, 4096)
        assert "profiles/skinny_rows.txt" in f.__doc__


@pytest.mark.parametrize("T", [33, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_layer_inside_the_context_makes_one_call_of_the_new_entry(monkeypatch, dt, T):
    dtype = S.DT[dt]
    m = _layer(520, 264, 50, dtype)
    rows, old = _count(monkeypatch)
    x = torch.randn(T, 1, 520, generator=torch.Generator().manual_seed(2)).to(DEV, dtype)
    with torch.no_grad(), sow_amd.skinny_rows(64):
        y = m(x)
    assert rows == [1] and old == [] and y.shape == (T, 1, 264)
    R._same(y.reshape(T, 264).cpu(), _cabi(m, x), "module against the C ABI")
    # outside the context the same call takes today's path: no skinny call, and the bits of the training forward
    del rows[:]
    with torch.no_grad():
        y0 = m(x)
    assert rows == [] and old == []
    yt = m(x.clone().requires_grad_(True))
    assert yt.requires_grad
    R._same(y0.cpu(), yt.detach().cpu(), "no-grad against the training forward, outside the context")


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "mxfp4"])
def test_quantised_stack_streams_codes_and_asks_for_no_image(monkeypatch, fmt):
    net = S._stack()
    assert quantize_accumulators(net, fmt=fmt) == 14
    x = torch.randn(48, 1, 512, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    _clear_qkv_ties(net, x)
    with _lib.switch(NO_SKINNY=1), torch.no_grad(), sow_amd.skinny_rows(64):
        ref = []
        net(x, ref)                     # the library refuses: the image and the existing path
    rows, old = _count(monkeypatch)
    key = (x.device, BF16)
    ops._ARENAS.pop(key, None)
    rec = []
    with torch.no_grad(), sow_amd.skinny_rows(64):
        out = net(x, rec)
    assert out.shape == (48, 1, 512) and len(rec) == 14
    assert rows == PATTERN and old == [], (rows, old)
    assert key not in ops._ARENAS, "an image was requested"
    for i, ((m, xin, y), (_, xref, yref)) in enumerate(zip(rec, ref)):
        R._same(y.reshape(-1, y.shape[-1]).cpu(), _cabi(m, xin), f"projection {i} against the C ABI")
        # ... and within the comparator of the NO_SKINNY run on the same input (the first projections share x bit for bit)
        if i < 3:
            assert torch.equal(E._bits(xin), E._bits(xref))
            d = dict(x=xin.reshape(-1, 512).cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(),
                     W=_image(m).cpu(), s=float(m.scale))
            S._check(f"rows_module_{fmt}_rows_{i}", BF16, d, y.reshape(-1, y.shape[-1]).cpu())
            # (tests/test_gpu_fp8_acc.py and test_gpu_fp4_acc.py ask of their NO_SKINNY runs a shape and finite values only; this
            # asks more, and says where its one extra term comes from.)
            assert yref.shape == y.shape and bool(torch.isfinite(yref).all())
            # The NO_SKINNY run is today's path for a short call: the dense product and the low-rank term are two kernels, so y
            # passes through memory once more in bf16 on the way.  That intermediate is x W^, h B or their sum, at most
            # |x W^| + |h B| in magnitude, and its rounding moves y by at most half a bf16 ulp of it, 2^-8 of that magnitude
            # (ulp(v) <= 2^-7 |v|).  The comparator's own bound plus that one term, nothing else:
            y_ref, y_sq, n_y = S._reference(BF16, d)
            x64, A64, B64, W64 = (to64(d[k]) for k in ("x", "A", "B", "W"))
            h64 = rne(d["s"] * (x64 @ A64), BF16)
            extra = 2.0 ** -8 * ((x64 @ W64).abs() + (h64 @ B64).abs())
            st = check_bound(yref.reshape(-1, yref.shape[-1]).cpu(), y_ref, bound(y_ref, BF16, fp32_floor(y_sq, n_y)) + extra,
                             name=f"rows_module_{fmt}_no_skinny_{i}: y")
            print(f"rows_module_{fmt}_no_skinny_{i}: worst err / (bound + one intermediate rounding) = {st['worst']:.3f}")


def test_unquantised_stack_and_what_keeps_todays_path(monkeypatch):
    net = S._stack()
    rows, old = _count(monkeypatch)
    x = torch.randn(64, 1, 512, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    _clear_qkv_ties(net, x)
    with torch.no_grad(), sow_amd.skinny_rows(64):
        rec = []
        net(x, rec)
        assert rows == PATTERN and old == []
        # every projection is the C-ABI call on its operands (which test_gpu_skinny_rows.py holds to float64); q / k / v of the
        # first block, whose input is x itself, are held to float64 here as well
        for i, (m, xin, y) in enumerate(rec):
            R._same(y.reshape(-1, y.shape[-1]).cpu(), _cabi(m, xin), f"projection {i} against the C ABI")
        S._check_projections(rec[:3], BF16, "rows_module_bf16")
        # T <= 32 inside the context: the existing entry, as before
        del rows[:]
        net(x[:17], [])
        assert rows == [] and old == PATTERN
        # T = 65: past the entry
        del old[:]
        net(torch.randn(65, 1, 512, device=DEV, dtype=BF16), [])
        assert rows == [] and old == []
        # a limit below T
        with sow_amd.skinny_rows(48):
            net(x, [])
        assert rows == [] and old == []
    # outside the context
    with torch.no_grad():
        net(x, [])
    assert rows == [] and old == []
    # grad enabled inside the context: the training path
    with sow_amd.skinny_rows(64):
        out = net(x.clone().requires_grad_(True), [])
    assert rows == [] and old == [] and out.requires_grad
    # a ragged layer and a low-rank accumulator inside the context
    xr = torch.randn(48, 516, device=DEV, dtype=BF16)
    for m, xin in ((_layer(516, 260, 8, BF16), xr), (_layer(520, 264, 8, BF16, acc="lowrank"), xr[:, :512].repeat(1, 2)[:, :520].contiguous())):
        with torch.no_grad():
            want = m(xin)
            with sow_amd.skinny_rows(64):
                got = m(xin)
        assert rows == [] and old == []
        R._same(got.cpu(), want.cpu(), "a layer the entry does not admit")


@pytest.mark.parametrize("group", [False, True], ids=["single", "qkv"])
@pytest.mark.parametrize("quant", [None, "fp8_e4m3", "mxfp4"], ids=["native", "e4m3", "mxfp4"])
def test_master_factors_under_autocast_take_the_new_entry(monkeypatch, quant, group):
    cd, d, r, T = BF16, 288, 16, 49
    net, _ = N._nets(d, r, cd, group, seed=9, quant=quant)
    rows, old = _count(monkeypatch)
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(2)).to(DEV, cd)
    with torch.no_grad(), torch.autocast("cuda", dtype=cd), sow_amd.skinny_rows(64):
        ys = [m(x) for m in net.layers()]
    assert rows == [len(net.names)] and old == [], (rows, old)
    for i, (m, y) in enumerate(zip(net.layers(), ys)):
        assert m.downscale_weights[0].dtype == F32 and y.dtype == cd
        R._same(y.cpu(), _cabi(m, x, flagged=True), f"projection {i} against the flagged C-ABI call")
