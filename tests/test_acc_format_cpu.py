"""What ops.check_accumulator, ops.acc_kind and ops.acc_logical_shape answer for the two quantised accumulator formats, on CPU
tensors (check_accumulator reaches its device check last), and the format table itself (sow_amd/acc_format.py).  Every expected
value is a literal read off include/sow_amd.h and the format definitions, not a recording of the code under test."""
import pytest
import torch

from sow_amd import _lib, ops

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
D_IN, D_OUT = 64, 16
FP8 = torch.float8_e4m3fn
# name: (kind, codes dtype, codes shape, scales dtype, scales shape, the other format's scale dtype, label)
FMTS = {"fp8_e4m3": (3, FP8, (64, 16), torch.int8, (16,), torch.uint8, "E4M3"),
        "mxfp4": (4, torch.uint8, (32, 16), torch.uint8, (2, 16), torch.int8, "MXFP4")}


def _pair(name, d_in=D_IN, d_out=D_OUT):
    _, cdt, _, sdt, _, _, _ = FMTS[name]
    if name == "mxfp4":
        return torch.zeros(d_in // 2, d_out, dtype=torch.uint8), torch.zeros(d_in // 32, d_out, dtype=sdt)
    return torch.zeros(d_in, d_out, dtype=F32).to(cdt), torch.zeros(d_out, dtype=sdt)


def _x(dtype=BF16, d_in=D_IN):
    return torch.zeros(4, d_in, dtype=dtype)


@pytest.mark.parametrize("name", list(FMTS))
def test_kind_and_logical_shape(name):
    codes, scales = _pair(name)
    assert tuple(codes.shape) == FMTS[name][2] and tuple(scales.shape) == FMTS[name][4]
    assert ops.acc_kind(codes, scales) == FMTS[name][0]
    assert ops.acc_kind(codes, None) == FMTS[name][0], "the codes dtype alone decides the kind"
    assert ops.acc_logical_shape(codes) == (64, 16)


@pytest.mark.parametrize("name", list(FMTS))
def test_type_errors_come_first(name):
    codes, scales = _pair(name)
    label, other = FMTS[name][6], FMTS[name][5]
    with pytest.raises(TypeError, match=label):
        ops.check_accumulator(_x(F32), D_IN, D_OUT, codes, scales)
    with pytest.raises(TypeError, match=label):
        ops.check_accumulator(_x(), D_IN, D_OUT, codes, scales, param_dtype=BF16)
    with pytest.raises(TypeError, match=label):
        ops.check_accumulator(_x(), D_IN, D_OUT, codes, None)
    with pytest.raises(TypeError, match=label):
        ops.check_accumulator(_x(), D_IN, D_OUT, codes, scales.to(other))
    # both defects at once: the dtype is reported, so the dtype checks run before the shape checks
    with pytest.raises(TypeError, match=label):
        ops.check_accumulator(_x(), D_IN, D_OUT, codes[:-1], scales.to(other))
    with pytest.raises(TypeError, match=label):
        ops.check_accumulator(_x(), D_IN, D_OUT, codes, scales.to(other)[..., :-1])


@pytest.mark.parametrize("name", list(FMTS))
def test_value_errors_for_shapes_and_multiples(name):
    codes, scales = _pair(name)
    label = FMTS[name][6]
    bad = [(codes[:-1], scales), (codes[:, :-1], scales), (codes, scales[..., :-1]), (codes, torch.cat([scales, scales]))]
    for c, s in bad:
        with pytest.raises(ValueError, match=label):
            ops.check_accumulator(_x(), D_IN, D_OUT, c, s)
    c12, s12 = _pair(name, d_out=12)           # matching shapes, out_features no multiple of 8
    with pytest.raises(ValueError, match=label):
        ops.check_accumulator(_x(), D_IN, 12, c12, s12)
    if name == "mxfp4":                        # matching halves, in_features no multiple of 32
        c48 = torch.zeros(24, D_OUT, dtype=torch.uint8)
        s48 = torch.zeros(1, D_OUT, dtype=torch.uint8)
        with pytest.raises(ValueError, match="MXFP4"):
            ops.check_accumulator(_x(d_in=48), 48, D_OUT, c48, s48)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("name", list(FMTS))
def test_well_formed_operands_reach_the_device_check(name, dtype):
    codes, scales = _pair(name)
    for kw in ({}, {"param_dtype": F32}, {"param_dtype": F32, "compute_dtype": dtype}):
        x = _x(F32 if "compute_dtype" in kw else dtype)
        with pytest.raises(RuntimeError, match="the accumulator is on cpu"):
            ops.check_accumulator(x, D_IN, D_OUT, codes, scales, **kw)


def test_unquantised_accumulators_as_before():
    x = _x()
    empty = torch.empty(0)
    W, Q, R = torch.zeros(D_IN, D_OUT, dtype=BF16), torch.zeros(D_IN, 6, dtype=BF16), torch.zeros(6, D_OUT, dtype=BF16)
    assert ops.acc_kind(None, None) == 0 and ops.acc_kind(empty, empty) == 0
    assert ops.acc_kind(W, None) == 2 and ops.acc_kind(W, empty) == 2 and ops.acc_kind(Q, R) == 1     # SOW_ACC_DENSE, _LOWRANK
    assert ops.check_accumulator(x, D_IN, D_OUT, None, None) == (0, 0)
    assert ops.check_accumulator(x, D_IN, D_OUT, empty, empty) == (0, 0)
    for down, up, exc, text in ((W.float(), None, TypeError, "dtype mismatch"), (W[:-1], None, ValueError, "dense accumulator must be"),
                                (Q, R[:-1], ValueError, "low-rank accumulator shapes"), (Q, R.float(), TypeError, "dtype mismatch"),
                                (W, None, RuntimeError, "the accumulator is on cpu"), (Q, R, RuntimeError, "the accumulator is on cpu")):
        with pytest.raises(exc, match=text):
            ops.check_accumulator(x, D_IN, D_OUT, down, up)
    # fp32 parameters: an fp32 or a native accumulator passes the dtype check, another half dtype does not
    for down in (W.float(), W):
        with pytest.raises(RuntimeError, match="the accumulator is on cpu"):
            ops.check_accumulator(x, D_IN, D_OUT, down, None, param_dtype=F32)
    with pytest.raises(TypeError, match="dtype mismatch"):
        ops.check_accumulator(x, D_IN, D_OUT, W.to(F16), None, param_dtype=F32)


def test_re_exports():
    assert ops.FP8 == FP8 and ops.FP4 == torch.uint8 and tuple(ops.CODES) == (FP8, torch.uint8) and ops.FP4_BLOCK == 32
    assert ops.skinny_fp8_pays(4, 4096, 4096) and ops.skinny_fp4_pays(32, 4096, 4096)
    assert not ops.skinny_fp8_pays(33, 4096, 4096) and not ops.skinny_fp4_pays(0, 4096, 4096)
    assert "profiles/fp8_acc.txt" in ops.skinny_fp8_pays.__doc__ and "profiles/fp4_acc.txt" in ops.skinny_fp4_pays.__doc__


@pytest.mark.parametrize("name", list(FMTS))
def test_table_row(name):
    from sow_amd import acc_format
    kind, cdt, cshape, sdt, sshape, _, label = FMTS[name]
    f = acc_format.FORMATS[name]
    assert acc_format.BY_CODE_DTYPE[cdt] is f and acc_format.BY_KIND[kind] is f
    assert (f.name, f.label, f.kind, f.code_dtype, f.scale_dtype) == (name, label, kind, cdt, sdt)
    assert f.code_shape(D_IN, D_OUT) == cshape and f.scale_shape(D_IN, D_OUT) == sshape
    codes, scales = _pair(name)
    assert f.logical_shape(codes) == (64, 16) and f.well_formed(codes, scales)
    assert not f.well_formed(codes, scales.to(FMTS[name][5])) and not f.well_formed(codes[:, :-1], scales)
    query, image = {"fp8_e4m3": ("sow_forward_skinny_fp8_workspace_bytes", "sow_acc_dequantize"),
                    "mxfp4": ("sow_forward_skinny_fp4_workspace_bytes", "sow_acc_dequantize_fp4")}[name]
    assert (f.workspace_query, f.dequantize) == (query, image) and query in _lib.SIGNATURES and image in _lib.SIGNATURES
    assert (f.rows_per_code, f.block, f.d_in_multiple, f.d_out_multiple) == {"fp8_e4m3": (1, None, 8, 8), "mxfp4": (2, 32, 32, 8)}[name]
    assert f.exp_range == {"fp8_e4m3": {BF16: (-117, 119), F16: (-15, 7)}, "mxfp4": {BF16: (-125, 125), F16: (-13, 13)}}[name]
    assert f.code_max == {"fp8_e4m3": 448.0, "mxfp4": 6.0}[name] and f.frexp[0] * 2.0 ** f.frexp[1] == f.code_max
    assert f.pays is {"fp8_e4m3": ops.skinny_fp8_pays, "mxfp4": ops.skinny_fp4_pays}[name]


def test_shape_message_names_only_what_is_enforced():
    """An E4M3 accumulator has no block: its ValueError names the shapes and the out_features multiple, nothing about in_features."""
    for name, tail in (("fp8_e4m3", "out_features a multiple of 8"), ("mxfp4", "in_features whole blocks of 32")):
        codes, scales = _pair(name)
        with pytest.raises(ValueError) as e:
            ops.check_accumulator(_x(), D_IN, D_OUT, codes[:-1], scales)
        text = str(e.value)
        assert text.endswith(tail) and str(FMTS[name][2]) in text and str(FMTS[name][4]) in text, text


def test_former_module_name_keeps_the_names_older_tests_import():
    from sow_amd import acc_quant, fp8_acc
    assert fp8_acc.quantize_tensor is acc_quant.quantize_tensor and fp8_acc.quantize_accumulators is acc_quant.quantize_accumulators
    assert "mxfp4" in fp8_acc.FORMATS and "fp8_e4m3" in fp8_acc.FORMATS
    W = (torch.arange(64 * 8).reshape(64, 8) % 13 - 6).to(BF16)
    for a, b in zip(fp8_acc.quantize_tensor_fp4(W), acc_quant.quantize_tensor(W, "mxfp4")):
        assert a.dtype == torch.uint8 and torch.equal(a, b)
    assert sorted(n for n in vars(fp8_acc) if not n.startswith("_")) == [
        "FORMATS", "quantize_accumulators", "quantize_tensor", "quantize_tensor_fp4"]
