"""-m gpu: the module surface of the short-row path on codes (sow_amd.short_rows + sow_amd.short_codes).  With both
opt-ins on, a SoWLinear whose accumulator is quantised routes forward + data gradient through ops.sow_forward_short_codes /
ops.sow_backward_short_codes where the format's pays_short keeps the call (3072 -> 768 at T = 100) and never calls ops.acc_operands:
no image, no arena.  The routed step equals the C-ABI call bit for bit (test_gpu_short_codes._run), single and as q / k / v
siblings, and stays within the float64 bounds of test_gpu_elementwise._check against a twin that holds W^.  With the new opt-in off
the calls recorded are those of test_gpu_short_rows_module: the image, then sow_forward_short."""
import pytest
import torch
import torch.nn as nn

import sow_amd
import test_gpu_elementwise as E
import test_gpu_short_codes as SC
import test_gpu_short_rows_module as SM
import test_gpu_skinny_rows_module as M
from sow_amd import ops, quantize_accumulators

pytestmark = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16
D_IN, D_OUT, R, T = 3072, 768, SM.R, 100      # a shape both formats' measured rules keep at 100 rows
FMT = {"fp8": "fp8_e4m3", "fp4": "mxfp4"}


def _inputs(dtype, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, D_IN, generator=g).to(SM.DEV, dtype), torch.randn(T, D_OUT, generator=g).to(SM.DEV, dtype)


class _Attn(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = (M._layer(D_IN, D_OUT, R, dtype, seed=11 + i) for i in range(3))

    def forward(self, x):
        return self.q_proj(x), self.k_proj(x), self.v_proj(x)


def _spy(monkeypatch):
    """Records, in call order, (name, layers in the call, hs) of ops.sow_forward_short_codes, ops.sow_backward_short_codes,
    ops.sow_forward_short and ops.acc_operands (the latter only when it is handed a quantised pair: an image would be built)."""
    rec = []
    f_codes, b_codes, f_short, acc_ops = ops.sow_forward_short_codes, ops.sow_backward_short_codes, ops.sow_forward_short, ops.acc_operands

    def fwd_codes(layers, save_h=True):
        res = f_codes(layers, save_h)
        rec.append(("fwd_codes", len(layers), None if res is None else res[1]))
        return res

    def bwd_codes(layers):
        rec.append(("bwd_codes", len(layers), None))
        return b_codes(layers)

    def fwd_short(layers, save_h=True):
        res = f_short(layers, save_h)
        rec.append(("fwd_short", len(layers), None if res is None else res[1]))
        return res

    def operands(accs, dtype):
        if any(d is not None and d.numel() and d.dtype in ops.BY_CODE_DTYPE for d, _ in accs):
            rec.append(("image", len(accs), None))
        return acc_ops(accs, dtype)

    for name, fn in (("sow_forward_short_codes", fwd_codes), ("sow_backward_short_codes", bwd_codes), ("sow_forward_short", fwd_short),
                     ("acc_operands", operands)):
        monkeypatch.setattr(ops, name, fn)
    return rec


def _quantised(fmt, dtype, seed):
    m = M._layer(D_IN, D_OUT, R, dtype, seed=seed)
    assert quantize_accumulators(nn.ModuleList([m]), fmt=FMT[fmt], strict=True) == 1
    return m


def _abi(fmt, dtype, m, x, dy):
    """The same step through the C ABI (test_gpu_short_codes._run, one run): (Case, operands, outputs)."""
    q, e = m.acc_downweight.data, m.acc_exponent
    d = dict(x=x.cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(), bias=m.bias.data.cpu(), dy=dy.cpu(),
             W=M._image(m).cpu(), q=(q.view(torch.uint8) if fmt == "fp8" else q).cpu(), e=e.cpu(), fmt=fmt)
    c = E.Case(f"short_codes_module_{fmt}", dtype, T, D_IN, D_OUT, R, acc="dense", bias=True, s=float(m.scale))
    (out,) = SC._run([(c, d)], runs=(0xFF,), what="C ABI")
    return c, d, out


@pytest.mark.parametrize("fmt,dt", [("fp8", "bf16"), ("fp4", "f16")])
def test_quantised_layer_reads_its_codes_in_place(monkeypatch, fmt, dt):
    dtype = SM.DT[dt]
    m = _quantised(fmt, dtype, 21)
    assert ops.FORMATS[FMT[fmt]].pays_short(T, D_IN, D_OUT), "the measured rule keeps this call"
    x, dy = _inputs(dtype)
    rec = _spy(monkeypatch)
    with sow_amd.short_rows(), sow_amd.short_codes():
        y, dx, dA, dB, dbias = SM._step(m, x, dy)
    assert [(k, n) for k, n, _ in rec] == [("fwd_codes", 1), ("bwd_codes", 1)] and rec[0][2] is not None, rec
    c, d, out = _abi(fmt, dtype, m, x, dy)
    got = dict(y=y, h=rec[0][2][0].view(T, 64), dx=dx, dA=dA, dB=dB, dbias=dbias)
    for k, v in got.items():
        SM._same(v.cpu(), out[k], f"{fmt} {dt}: {k} against the C-ABI call")
    # within the float64 bounds on W^, the accumulator of the twin
    SC._check(c, d, {k: v.cpu() for k, v in got.items()})
    # a no-grad call of the same rows: the forward on the codes with h_save = NULL, the same y
    del rec[:]
    with torch.no_grad(), sow_amd.short_rows(), sow_amd.short_codes():
        y0 = m(x)
    assert [(k, n, h) for k, n, h in rec] == [("fwd_codes", 1, [None])], rec
    SM._same(y0, y, "no-grad forward against the training forward")


def test_with_the_new_opt_in_off_the_calls_are_todays(monkeypatch):
    """Inside short_rows alone -- and with short_codes on but outside short_rows -- a quantised layer builds its image (forward and
    backward) and, inside short_rows, hands it to sow_forward_short: what test_gpu_short_rows_module pins.  The results are those of the
    twin that holds W^, bit for bit, and the codes path reproduces dX bit for bit (the data phase's identity) on the module surface too."""
    m = _quantised("fp8", BF16, 21)
    twin = M._layer(D_IN, D_OUT, R, BF16, seed=21)
    with torch.no_grad():
        twin.acc_downweight.copy_(M._image(m))
        twin.downscale_weights[0].copy_(m.downscale_weights[0])
    x, dy = _inputs(BF16)
    rec = _spy(monkeypatch)
    with sow_amd.short_rows():
        off = SM._step(m, x, dy)
        want = SM._step(twin, x, dy)
    assert [(k, n) for k, n, _ in rec] == [("image", 1), ("fwd_short", 1), ("image", 1), ("fwd_short", 1)], rec
    for g, w, k in zip(off, want, ("y", "dx", "dA", "dB", "dbias")):
        SM._same(g, w, f"short_rows alone: {k} against the twin")
    del rec[:]
    with sow_amd.short_codes():
        outside = SM._step(m, x, dy)
    assert [(k, n) for k, n, _ in rec] == [("image", 1), ("image", 1)], rec
    explicit = SM._explicit(twin, x, dy)
    for g, w, k in zip(outside, explicit, ("y", "dx", "dA", "dB", "dbias")):
        SM._same(g, w, f"short_codes outside short_rows: {k} against today's path")
    with sow_amd.short_rows(), sow_amd.short_codes():
        on = SM._step(m, x, dy)
    SM._same(on[1], off[1], "dX on the codes against dX on the image")


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_qkv_group_on_codes(monkeypatch, fmt):
    """ONE sow_forward_short_codes call and one sow_backward_short_codes call for three quantised siblings, no image; every y, dA, dB,
    dbias is what the sibling's single call gives (held to the C ABI above), dX their data gradients summed last sibling first."""
    net = _Attn(BF16)
    assert quantize_accumulators(net, fmt=FMT[fmt], strict=True) == 3
    x, _ = _inputs(BF16)
    g = torch.Generator().manual_seed(5)
    dys = tuple(torch.randn(T, D_OUT, generator=g).to(SM.DEV, BF16) for _ in range(3))
    assert sow_amd.group_siblings(net) == 1
    rec = _spy(monkeypatch)
    with sow_amd.short_rows(), sow_amd.short_codes():
        ys, dx, grads = SM._group_step(net, x, dys)
    assert [(k, n) for k, n, _ in rec] == [("fwd_codes", 3), ("bwd_codes", 3)], rec
    sow_amd.ungroup_siblings(net)
    singles = []
    with sow_amd.short_rows(), sow_amd.short_codes():
        for m, dy in zip(net.children(), dys):
            singles.append(SM._step(m, x, dy))
    assert [(k, n) for k, n, _ in rec[2:]] == [("fwd_codes", 1), ("bwd_codes", 1)] * 3, rec
    for i, (s, y, g3) in enumerate(zip(singles, ys, grads)):
        for a, b, k in zip((y, *g3), (s[0], s[2], s[3], s[4]), ("y", "dA", "dB", "dbias")):
            SM._same(a, b, f"sibling {i}: {k}")
    want = singles[2][1] + singles[1][1]
    SM._same(dx, want + singles[0][1], "dX: the siblings' data gradients, summed last sibling first")
