"""-m gpu: the module surface of the short-row path (sow_amd.short_rows).  Inside the context SoWLinear and a q / k / v
SiblingGroup route forward + data gradient through sow_forward_short / sow_backward_short where ops.short_rows_pays keeps the
call (768 -> 768 at T = 100), and stay on today's path where the measured rule excludes it (T = 1024: bit-identical to the call
outside the context); outside the context nothing changes.  The routed layer is held to float64 by test_gpu_elementwise._check
(the h_save it compares is the one the forward handed to autograd); the group to its siblings' single calls, bit for bit."""
import pytest
import torch
import torch.nn as nn

import sow_amd
import test_gpu_elementwise as E
import test_gpu_skinny_rows_module as M
from sow_amd import ops, quantize_accumulators

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DT = {"bf16": BF16, "f16": F16}
D, R = 768, 8


def _spy(monkeypatch):
    """Records what ops.sow_forward_short returns: one (layers in the call, hs) per call."""
    rec, orig = [], ops.sow_forward_short

    def fwd(layers, save_h=True):
        res = orig(layers, save_h)
        rec.append((len(layers), None if res is None else res[1]))
        return res

    monkeypatch.setattr(ops, "sow_forward_short", fwd)
    return rec


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(E._bits(a), E._bits(b)), f"{what}: {int((E._bits(a) != E._bits(b)).sum())} elements differ"


def _inputs(T, dtype, d_out=D, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, D, generator=g).to(DEV, dtype), torch.randn(T, d_out, generator=g).to(DEV, dtype)


def _step(m, x, dy):
    """(y, dx, dA, dB, dbias) of one forward + backward of the module m."""
    for p in m.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    y = m(xin)
    y.backward(dy)
    return (y.detach(), xin.grad, m.downscale_weights[0].grad, m.upscale_weights[0].grad, m.bias.grad)


def _explicit(m, x, dy):
    """The same step through ops.sow_forward / ops.sow_backward: today's path, whatever the context says."""
    A, B, W = m.downscale_weights[0].data, m.upscale_weights[0].data, m.acc_downweight.data
    y, h = ops.sow_forward(x, A, B, W, None, m.bias.data, float(m.scale))
    dx, dA, dB, dbias = ops.sow_backward(dy, x, h, A, B, W, None, float(m.scale), True)
    return y, dx, dA, dB, dbias


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_layer_at_100_rows_takes_the_new_pair_and_meets_float64(monkeypatch, dt):
    dtype = DT[dt]
    m = M._layer(D, D, R, dtype)
    x, dy = _inputs(100, dtype)
    rec = _spy(monkeypatch)
    with sow_amd.short_rows():
        y, dx, dA, dB, dbias = _step(m, x, dy)
    assert [n for n, _ in rec] == [1] and rec[0][1] is not None, "one sow_forward_short call, admitted"
    c = E.Case(f"short_module_{dt}", dtype, 100, D, D, R, acc="dense", bias=True, s=float(m.scale))
    d = dict(x=x.cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(), bias=m.bias.data.cpu(), dy=dy.cpu(),
             W=m.acc_downweight.data.cpu())
    E._check(c, d, dict(y=y.cpu(), h=rec[0][1][0].view(100, 64).cpu(), dx=dx.cpu(), dA=dA.cpu(), dB=dB.cpu(), dbias=dbias.cpu()))
    # a no-grad call of the same rows: the forward with h_save = NULL, the same y
    del rec[:]
    with torch.no_grad(), sow_amd.short_rows():
        y0 = m(x)
    assert [n for n, _ in rec] == [1] and rec[0][1] == [None]
    _same(y0, y, "no-grad forward against the training forward")


@pytest.mark.parametrize("T", [100, 1024])
def test_outside_the_context_nothing_changes(monkeypatch, T):
    """The default is off: the module step is the explicit ops.sow_forward / sow_backward step, bit for bit, and no call of the new
    entry is made.  At T = 1024 the same holds INSIDE the context: the measured rule excludes the row count."""
    m = M._layer(D, D, R, BF16)
    x, dy = _inputs(T, BF16)
    rec = _spy(monkeypatch)
    want = _explicit(m, x, dy)
    got = _step(m, x, dy)
    assert rec == []
    for g, w, k in zip(got, want, ("y", "dx", "dA", "dB", "dbias")):
        _same(g, w, f"T = {T}, outside the context: {k}")
    if T == 1024:
        assert not ops.short_rows_pays(T, D, D)
        with sow_amd.short_rows():
            inside = _step(m, x, dy)
        assert rec == []
        for g, w, k in zip(inside, want, ("y", "dx", "dA", "dB", "dbias")):
            _same(g, w, f"T = 1024, inside the context: {k}")


class _Attn(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = (M._layer(D, D, R, dtype, seed=11 + i) for i in range(3))

    def forward(self, x):
        return self.q_proj(x), self.k_proj(x), self.v_proj(x)


def _group_step(net, x, dys):
    for p in net.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    ys = net(xin)
    torch.autograd.backward(ys, dys)
    return [y.detach() for y in ys], xin.grad, [(m.downscale_weights[0].grad, m.upscale_weights[0].grad, m.bias.grad) for m in net.children()]


@pytest.mark.parametrize("T", [100, 1024])
def test_qkv_group_inside_the_context(monkeypatch, T):
    """T = 100: ONE sow_forward_short call for the three siblings; every y, dA, dB, dbias is what the sibling's single call gives
    (which the test above holds to float64), and dX is their data gradients summed last sibling first.  T = 1024: the rule keeps
    today's grouped path, bit for bit."""
    net = _Attn(BF16)
    x, _ = _inputs(T, BF16)
    g = torch.Generator().manual_seed(5)
    dys = tuple(torch.randn(T, D, generator=g).to(DEV, BF16) for _ in range(3))
    assert sow_amd.group_siblings(net) == 1
    outside = _group_step(net, x, dys)
    rec = _spy(monkeypatch)
    with sow_amd.short_rows():
        ys, dx, grads = _group_step(net, x, dys)
    if T == 1024:
        assert rec == []
        for a, b in zip(ys + [dx] + [t for g3 in grads for t in g3], outside[0] + [outside[1]] + [t for g3 in outside[2] for t in g3]):
            _same(a, b, "T = 1024: the grouped path of today")
        return
    assert [n for n, _ in rec] == [3]
    sow_amd.ungroup_siblings(net)
    singles = []
    with sow_amd.short_rows():
        for m, dy in zip(net.children(), dys):
            singles.append(_step(m, x, dy))
    assert [n for n, _ in rec] == [3, 1, 1, 1]
    for i, (s, y, g3) in enumerate(zip(singles, ys, grads)):
        for a, b, k in zip((y, *g3), (s[0], s[2], s[3], s[4]), ("y", "dA", "dB", "dbias")):
            _same(a, b, f"sibling {i}: {k}")
    want = singles[2][1] + singles[1][1]
    _same(dx, want + singles[0][1], "dX: the siblings' data gradients, summed last sibling first")


def test_e4m3_layer_equals_its_unquantised_twin(monkeypatch):
    """A quantised layer passes its image W^ as today: inside the context it is the layer that holds W^, bit for bit."""
    m = M._layer(D, D, R, BF16, seed=21)
    twin = M._layer(D, D, R, BF16, seed=21)
    assert quantize_accumulators(nn.ModuleList([m]), fmt="fp8_e4m3", strict=True) == 1
    with torch.no_grad():
        twin.acc_downweight.copy_(M._image(m))
        twin.downscale_weights[0].copy_(m.downscale_weights[0])     # (A comes from the module's own initialiser)
    x, dy = _inputs(100, BF16)
    rec = _spy(monkeypatch)
    with sow_amd.short_rows():
        got, want = _step(m, x, dy), _step(twin, x, dy)
    assert [n for n, _ in rec] == [1, 1]
    for g, w, k in zip(got, want, ("y", "dx", "dA", "dB", "dbias")):
        _same(g, w, f"E4M3 layer against its twin: {k}")
