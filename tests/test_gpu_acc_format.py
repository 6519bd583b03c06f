"""-m gpu: what the Python call paths answer for the two quantised accumulator formats at the smallest shape both admit --
T = 1, d_in = 32 (one MXFP4 block), d_out = 8 (one 8-column vector), r = 2 -- in bf16 and f16: admission, refusals, exception
classes, and outputs bit-identical to the dense path on the image.  The operands are small integers and halves, so every fp32
sum of either path is exact and the two paths must agree to the bit whatever their summation order."""
import pytest
import torch
import torch.nn as nn

import fp4_acc_ref as R4
import fp8_acc_ref as R8
from sow_amd import SoWLinear, group_siblings, ops, quantize_accumulators
from sow_amd import group as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
T, D_IN, D_OUT, RANK = 1, 32, 8, 2
FMTS = ("fp8_e4m3", "mxfp4")
OTHER_SCALE = {"fp8_e4m3": torch.uint8, "mxfp4": torch.int8}


def _ints(shape, lo, hi, seed, dtype, step=1.0):
    return (torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float() * step).to(DEV, dtype)


def _operands(fmt, dtype, d_in=D_IN, seed=0):
    """x, A, B, bias and the (codes, scales) pair of a small-integer W, through the integer references."""
    W = _ints((d_in, D_OUT), -3, 3, seed + 4, dtype).cpu()
    if fmt == "mxfp4":
        codes, scales = R4.quantize(W)
    else:
        codes, scales = R8.quantize(W)
        codes = codes.view(torch.float8_e4m3fn)
    return dict(x=_ints((T, d_in), -1, 1, seed, dtype), A=_ints((d_in, RANK), -1, 1, seed + 1, dtype),
                B=_ints((RANK, D_OUT), -2, 2, seed + 2, dtype, 0.5), bias=_ints((D_OUT,), -4, 4, seed + 3, dtype, 0.25),
                codes=codes.to(DEV), scales=scales.to(DEV))


def _admits(o, **kw):
    d = dict(o, **kw)
    return ops.skinny_admits(d["x"], d["A"], d["B"], d["codes"], d["scales"], d["bias"], mixed=d.get("mixed", False))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_skinny_admits(fmt, dtype):
    o = _operands(fmt, dtype)
    assert _admits(o) is True
    assert _admits(o, scales=o["scales"].to(OTHER_SCALE[fmt])) is False
    assert _admits(o, scales=o["scales"][..., :-1]) is False
    assert _admits(o, scales=torch.cat([o["scales"], o["scales"]])) is False
    assert _admits(o, scales=None) is False
    assert _admits(o, mixed=True) is False, "mixed=True needs fp32 factors"
    assert _admits(o, mixed=True, A=o["A"].float(), B=o["B"].float(), bias=o["bias"].float()) is True
    assert ops.skinny_acc(o["codes"], o["scales"]) == (o["codes"], o["scales"])


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_skinny_admits_whole_mxfp4_blocks_only(dtype):
    o = _operands("fp8_e4m3", dtype, d_in=40)          # 40 is a multiple of 8, not of 32
    codes = torch.full((20, D_OUT), 0x22, dtype=torch.uint8, device=DEV)
    scales = torch.full((1, D_OUT), 127, dtype=torch.uint8, device=DEV)
    assert _admits(o, codes=codes, scales=scales) is False
    assert _admits(o, codes=codes, scales=torch.cat([scales, scales])) is False
    assert _admits(_operands("fp8_e4m3", dtype, d_in=40)) is True


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_forward_skinny_equals_dense_path_on_the_image(fmt, dtype):
    o = _operands(fmt, dtype)
    img = ops.acc_dequantize(o["codes"], o["scales"], dtype)
    assert img.dtype == dtype and tuple(img.shape) == (D_IN, D_OUT) and ops.acc_logical_shape(o["codes"]) == (D_IN, D_OUT)
    ys = ops.sow_forward_skinny([(o["x"], o["A"], o["B"], (o["codes"], o["scales"]), o["bias"], 0.5)])
    want, _ = ops.sow_forward(o["x"], o["A"], o["B"], img, None, o["bias"], 0.5, save_h=False)
    assert ys is not None and len(ys) == 1 and ys[0].dtype == dtype
    assert torch.equal(ys[0].view(torch.int16), want.view(torch.int16))
    exact = (o["x"].double() @ img.double() + 0.5 * (o["x"].double() @ o["A"].double()) @ o["B"].double() + o["bias"].double())
    assert torch.equal(ys[0], exact.to(dtype)), "every sum is exact in fp32: y is the exact value, rounded once"
    assert float(ys[0].float().abs().max()) > 0
    for bad in (o["scales"].to(OTHER_SCALE[fmt]), o["scales"][..., :-1], torch.cat([o["scales"], o["scales"]])):
        with pytest.raises(TypeError):
            ops.sow_forward_skinny([(o["x"], o["A"], o["B"], (o["codes"], bad), o["bias"], 0.5)])


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_forward_skinny_refuses_a_partial_mxfp4_block(dtype):
    """Codes [20, 8] with scales [1, 8] stand for 40 rows, of which the block scale covers 32: not a pair of the format, TypeError
    as in acc_dequantize.  (Before the format table this one case slipped through a `// 16` and came back as None.)"""
    o = _operands("fp8_e4m3", dtype, d_in=40)
    codes = torch.full((20, D_OUT), 0x22, dtype=torch.uint8, device=DEV)
    scales = torch.full((1, D_OUT), 127, dtype=torch.uint8, device=DEV)
    with pytest.raises(TypeError):
        ops.sow_forward_skinny([(o["x"], o["A"], o["B"], (codes, scales), o["bias"], 0.5)])
    with pytest.raises(TypeError):
        ops.acc_dequantize(codes, scales, dtype)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("fmt", FMTS)
def test_acc_dequantize_refusals(fmt, dtype):
    o = _operands(fmt, dtype)
    codes, scales = o["codes"], o["scales"]
    for bad in (scales.to(OTHER_SCALE[fmt]), scales[..., :-1], torch.cat([scales, scales])):
        with pytest.raises(TypeError):
            ops.acc_dequantize(codes, bad, dtype)
    with pytest.raises(TypeError):
        ops.acc_dequantize(codes, scales, F32)
    for shape in ((D_IN, D_OUT + 8), (D_IN // 2, D_OUT), (D_IN * D_OUT,)):
        with pytest.raises(ValueError):
            ops.acc_dequantize(codes, scales, dtype, out=torch.empty(shape, dtype=dtype, device=DEV))
    with pytest.raises(ValueError):
        ops.acc_dequantize(codes, scales, dtype, out=torch.empty((D_IN, D_OUT), dtype=F16 if dtype == BF16 else BF16, device=DEV))
    out = torch.empty((D_IN, D_OUT), dtype=dtype, device=DEV)
    assert ops.acc_dequantize(codes, scales, dtype, out=out) is out
    assert torch.equal(out.view(torch.int16), ops.acc_dequantize(codes, scales, dtype).view(torch.int16))


class _Mlp(nn.Module):
    """gate / up siblings on one input, 32 -> 8, r = 2, small-integer operands."""

    def __init__(self, dtype):
        super().__init__()
        self.mlp = nn.Module()
        for i, nm in enumerate(("gate_proj", "up_proj")):
            m = SoWLinear(D_IN, D_OUT, bias=True, rank=RANK, init_method="normal", scale=0.5, device=DEV, dtype=dtype)
            with torch.no_grad():
                m.downscale_weights[0].copy_(_ints((D_IN, RANK), -1, 1, 10 + i, dtype))
                m.upscale_weights[0].copy_(_ints((RANK, D_OUT), -2, 2, 20 + i, dtype, 0.5))
                m.bias.copy_(_ints((D_OUT,), -4, 4, 30 + i, dtype, 0.25))
            m.acc_downweight = nn.Parameter(_ints((D_IN, D_OUT), -3, 3, 50 + i, dtype), requires_grad=False)
            setattr(self.mlp, nm, m)

    def layers(self):
        return [self.mlp.gate_proj, self.mlp.up_proj]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_siblings_of_two_formats_run_per_layer(dtype):
    net = _Mlp(dtype)
    gate, up = net.layers()
    assert quantize_accumulators(gate, fmt="fp8_e4m3", strict=True) == 1 and quantize_accumulators(up, fmt="mxfp4", strict=True) == 1
    assert gate.acc_downweight.dtype == torch.float8_e4m3fn and gate.acc_exponent.dtype == torch.int8
    assert up.acc_downweight.dtype == torch.uint8 and tuple(up.acc_downweight.shape) == (16, 8) and tuple(up.acc_exponent.shape) == (1, 8)
    x = _ints((T, D_IN), -1, 1, 7, dtype)
    with torch.no_grad():
        singles = [m(x) for m in (gate, up)]
    assert group_siblings(net) == 1
    with torch.no_grad():
        assert gate._sibling_group._forward_skinny(x) is G._PER_LAYER
        grouped = [m(x) for m in (gate, up)]
    for a, b in zip(grouped, singles):
        assert a.shape == (T, D_OUT) and torch.equal(a.view(torch.int16), b.view(torch.int16))
    # two siblings of ONE format are one call of the library
    net2 = _Mlp(dtype)
    assert quantize_accumulators(net2, fmt="mxfp4", strict=True) == 2 and group_siblings(net2) == 1
    with torch.no_grad():
        ys = net2.layers()[0]._sibling_group._forward_skinny(x)
    assert isinstance(ys, list) and len(ys) == 2
