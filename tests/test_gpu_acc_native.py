"""-m gpu: fp32 master factors over an accumulator of the compute dtype -- include/sow_amd.h SOW_ACC_NATIVE (next to
SOW_PARAM_F32), the skinny forward with fp32 factors, SoWLinear under torch.autocast after sow_amd.master_factors.

Every expectation is an equality of bits; nothing here has a tolerance.
* C ABI: a call with  cd | SOW_PARAM_F32 | SOW_ACC_NATIVE  (fp32 A, B, bias; accumulator of cd, read in place; workspace of
  exactly the flagged query, a guard behind it) equals the SOW_PARAM_F32 call on the fp32 copy of the accumulator in y, h_save,
  dx, dA, dB and dbias, and the unflagged call on pre-rounded parameters in y, h_save and dx.
* Skinny: the flagged call equals the unflagged call on pre-rounded factors for every kind (none, dense, E4M3, MXFP4).
* Module: under autocast a layer with fp32 factors over a bf16 / f16 or quantised base equals its twin on the existing path.
The fp32 factors and biases of every case hold values that are NOT numbers of the compute dtype, exact rounding midpoints in
both tie directions among them (_master; asserted on the CPU): an instantiation that truncates, or skips the rounding, fails.
The accumulators hold numbers of the compute dtype, so their fp32 copy is exact."""
import copy

import pytest
import torch
import torch.nn as nn

import graph_replay as GR
import test_gpu_elementwise as E
from sow_amd import (FactorBucket, SoWLinear, _lib, dequantize_accumulators, factor_parameters, acc_quant, group_siblings, ops,
                     quantize_accumulators)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {"bf16": BF16, "f16": F16}
CODE = {BF16: _lib.BF16, F16: _lib.F16}
PF = _lib.PARAM_F32
NATIVE = getattr(_lib, "ACC_NATIVE", 0x800)     # (the parent has no such bit: the calls below then fail with SOW_ERR_DTYPE)
GUARD_BYTE = 0xA5


def _bits(t):
    return E._bits(t)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {diff.numel()} elements differ"


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def _master(shape, std, cd, g):
    """fp32 values around numbers of cd (v, and its neighbour away from zero n): element i holds, by i mod 4, the exact
    midpoint (v + n) / 2 -- a tie: to v when v's last bit is even, to n when it is odd --, v + (n - v) / 4 (rounds to v),
    v + 3 (n - v) / 4 (rounds to n), or v itself.  Checked: .to(cd) changes at least half of the elements, ties go both ways."""
    v = (torch.randn(shape, generator=g) * std).to(cd)
    v = torch.where(v == 0, torch.ones_like(v), v)
    n = (v.view(torch.int16) + 1).view(cd)            # the same sign, one unit in the last place further from zero
    vf, nf = v.float().flatten(), n.float().flatten()
    sel = torch.arange(vf.numel()) % 4
    out = torch.where(sel == 0, (vf + nf) / 2, torch.where(sel == 1, vf + (nf - vf) / 4, torch.where(sel == 2, vf + 3 * (nf - vf) / 4, vf)))
    out = out.view(shape)
    assert out.dtype == F32 and bool(torch.isfinite(out).all())
    rounded = out.to(cd).float()
    assert float((rounded != out).float().mean()) >= 0.5, "at least half of the elements are no numbers of the compute dtype"
    if out.numel() >= 16:
        tie = (sel == 0).view(shape)
        down, up = tie & (rounded.abs() < out.abs()), tie & (rounded.abs() > out.abs())
        assert bool(down.any()) and bool(up.any()), "ties to the even neighbour below and to the even neighbour above"
        assert bool((down | up)[tie].all())
    return out


def _operands(cd, T, d_in, d_out, r, bias, acc, r_acc=0, seed=0):
    """CPU operands of one layer: x, dy and the accumulator in cd, fp32 master A, B, bias."""
    g = torch.Generator().manual_seed(9000 + 131 * seed + T + 7 * r + r_acc)
    d = dict(x=torch.randn(T, d_in, generator=g).to(cd), dy=torch.randn(T, d_out, generator=g).to(cd),
             A=_master((d_in, r), 0.05, cd, g), B=_master((r, d_out), 0.05, cd, g),
             bias=_master((d_out,), 0.1, cd, g) if bias else None, acc_down=None, acc_up=None)
    if acc == "dense":
        d["acc_down"] = (torch.randn(d_in, d_out, generator=g) * 0.02).to(cd)
    elif acc == "lowrank":
        d["acc_down"] = (torch.randn(d_in, r_acc, generator=g) * 0.05).to(cd)
        d["acc_up"] = (torch.randn(r_acc, d_out, generator=g) * 0.05).to(cd)
    return d


def _dev(t, dtype=None):
    return None if t is None else t.to(DEV, dtype if dtype is not None else t.dtype).contiguous()


def _form(d, cd, form):
    """The device tensors a call of `form` reads: "native" (fp32 factors, accumulator of cd), "legacy" (everything fp32) or
    "plain" (everything pre-rounded to cd).  x and dy are of cd in all three."""
    pdt = cd if form == "plain" else F32
    adt = F32 if form == "legacy" else cd
    return dict(x=_dev(d["x"]), dy=_dev(d["dy"]), A=_dev(d["A"], pdt), B=_dev(d["B"], pdt), bias=_dev(d["bias"], pdt),
                acc_down=_dev(d["acc_down"], adt), acc_up=_dev(d["acc_up"], adt))


def _code(cd, form):
    return CODE[cd] | {"native": PF | NATIVE, "legacy": PF, "plain": 0}[form]


class _Ws:
    """A workspace of exactly `nbytes` with a guard behind it."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 256,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.buf[:self.n] = 0xFF

    def ptr(self):
        return self.buf.data_ptr() if self.n else None

    def check(self, what):
        assert bool((self.buf[self.n:] == GUARD_BYTE).all()), f"{what}: written past the queried workspace"


def _kind(d):
    return _lib.ACC_NONE if d["acc_down"] is None else _lib.ACC_LOWRANK if d["acc_up"] is not None else _lib.ACC_DENSE


def _outputs(cd, form, T, d_in, d_out, r, bias):
    gdt = cd if form == "plain" else F32
    hcols = 64 if r <= 64 else r
    new = lambda shape, dt: torch.full(shape, float("nan"), dtype=dt, device=DEV)      # noqa: E731
    return dict(y=new((T, d_out), cd), h=new((T, hcols), cd), dx=new((T, d_in), cd), dA=new((d_in, r), gdt), dB=new((r, d_out), gdt),
                dbias=new((d_out,), gdt) if bias else None)


def _layer_args(a, p, o, T, d_in, d_out, r, r_acc, kind, s, ws):
    a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias = (E._ptr(p[k]) for k in ("x", "A", "B", "acc_down", "acc_up", "bias"))
    a.y, a.h_save, a.dy, a.dx, a.dA, a.dB, a.dbias = (E._ptr(t) for t in (o["y"], o["h"], p["dy"], o["dx"], o["dA"], o["dB"], o["dbias"]))
    a.T, a.d_in, a.d_out, a.r_live, a.r_acc, a.acc_kind, a.scale, a.grad_beta = T, d_in, d_out, r, r_acc, kind, s, 0.0
    a.workspace, a.workspace_bytes = ws.ptr(), ws.n


def _single(d, cd, form, s=0.5):
    """sow_forward + sow_backward_ex(DATA | WEIGHTS) through the C ABI, each with a workspace of exactly its query."""
    lib = _lib.load()
    T, d_in = d["x"].shape
    r, d_out = d["B"].shape
    kind, r_acc = _kind(d), (d["acc_down"].shape[1] if d["acc_up"] is not None else 0)
    code = _code(cd, form)
    p = _form(d, cd, form)
    o = _outputs(cd, form, T, d_in, d_out, r, d["bias"] is not None)
    fws = _Ws(lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, code))
    bws = _Ws(lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, code))
    if form != "plain":
        assert fws.n > 0 and bws.n > 0, "the flagged queries are never 0"
    st = E._stream()
    _lib.check(lib.sow_forward(E._ptr(p["x"]), E._ptr(p["A"]), E._ptr(p["B"]), E._ptr(p["acc_down"]), E._ptr(p["acc_up"]),
                               E._ptr(p["bias"]), E._ptr(o["y"]), E._ptr(o["h"]), T, d_in, d_out, r, r_acc, kind, s, code, fws.ptr(),
                               fws.n, st), f"sow_forward ({form})")
    _lib.check(lib.sow_backward_ex(E._ptr(p["dy"]), E._ptr(p["x"]), E._ptr(o["h"]), E._ptr(p["A"]), E._ptr(p["B"]),
                                   E._ptr(p["acc_down"]), E._ptr(p["acc_up"]), E._ptr(o["dx"]), E._ptr(o["dA"]), E._ptr(o["dB"]),
                                   E._ptr(o["dbias"]), T, d_in, d_out, r, r_acc, kind, s, 0.0, code, bws.ptr(), bws.n,
                                   _lib.BWD_DATA | _lib.BWD_WEIGHTS, st), f"sow_backward_ex ({form})")
    torch.cuda.synchronize()
    fws.check(f"forward ({form})"), bws.check(f"backward ({form})")
    return o


def _compare(native, legacy, plain, what):
    for k in ("y", "h", "dx", "dA", "dB", "dbias"):
        if native[k] is not None:
            _same(native[k], legacy[k], f"{what}: {k} against SOW_PARAM_F32 on the fp32 copy of the accumulator")
    for k in ("y", "h", "dx"):
        _same(native[k], plain[k], f"{what}: {k} against the unflagged call on pre-rounded parameters")
    assert bool(torch.isfinite(native["y"].float()).all()) and float(native["dx"].float().abs().max()) > 0


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------------
SHAPES = [  # (T, d_in, d_out, r, accumulator, r_acc)
    (64, 512, 512, 50, "dense", 0),        # dense, the short / one-launch path
    (8193, 512, 1376, 8, "dense", 0),      # dense, streaming, odd T
    (256, 768, 768, 100, "dense", 0),      # dense, wide rank
    (256, 512, 512, 50, "lowrank", 100),   # low-rank
]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"T{s[0]}_{s[1]}x{s[2]}_r{s[3]}_{s[4]}{s[5] or ''}")
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_cabi_forward_backward(dt, shape, bias):
    cd = DT[dt]
    T, d_in, d_out, r, acc, r_acc = shape
    d = _operands(cd, T, d_in, d_out, r, bias, acc, r_acc)
    native, legacy, plain = (_single(d, cd, form) for form in ("native", "legacy", "plain"))
    _compare(native, legacy, plain, f"{dt} {shape}")
    assert native["dA"].dtype == F32 and native["dB"].dtype == F32


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_cabi_group_of_three_siblings(dt):
    """sow_forward_group / sow_backward_group on three siblings of the first shape (one x), every workspace of exactly the
    flagged query."""
    lib = _lib.load()
    cd = DT[dt]
    T, d_in, d_out, r, acc, r_acc = SHAPES[0]
    ds = [_operands(cd, T, d_in, d_out, r, i != 1, acc, r_acc, seed=10 + i) for i in range(3)]
    for d in ds[1:]:
        d["x"] = ds[0]["x"]
    res = {}
    for form in ("native", "legacy", "plain"):
        code = _code(cd, form)
        x = _dev(ds[0]["x"])
        arr = (_lib.LayerArgs * 3)()
        outs, keep = [], []
        for i, d in enumerate(ds):
            p = dict(_form(d, cd, form), x=x)
            o = _outputs(cd, form, T, d_in, d_out, r, d["bias"] is not None)
            ws = _Ws(lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, _lib.ACC_DENSE, code))
            _layer_args(arr[i], p, o, T, d_in, d_out, r, r_acc, _lib.ACC_DENSE, 0.5, ws)
            outs.append(o), keep.append((p, ws))
        _lib.check(lib.sow_forward_group(arr, 3, code, E._stream()), f"sow_forward_group ({form})")
        _lib.check(lib.sow_backward_group(arr, 3, code, _lib.BWD_DATA | _lib.BWD_WEIGHTS, E._stream()), f"sow_backward_group ({form})")
        torch.cuda.synchronize()
        for _, ws in keep:
            ws.check(f"group ({form})")
        res[form] = outs
    for i in range(3):
        _compare(res["native"][i], res["legacy"][i], res["plain"][i], f"{dt} sibling {i}")


# ---- 2. the skinny forward with fp32 factors ------------------------------------------------------------------------------------------
KINDS = {"none": _lib.ACC_NONE, "dense": _lib.ACC_DENSE, "e4m3": _lib.ACC_DENSE_FP8, "mxfp4": _lib.ACC_DENSE_FP4}


def _skinny_layer(cd, kind, T, d_in, d_out, r, bias, seed=0):
    """CPU / device operands of one skinny layer: fp32 master factors, the accumulator as the kind stores it."""
    d = _operands(cd, T, d_in, d_out, r, bias, "dense" if kind != "none" else None, seed=seed)
    acc_down, acc_up = _dev(d["acc_down"]), None
    if kind == "e4m3":
        acc_down, acc_up = acc_quant.quantize_tensor(acc_down)
    elif kind == "mxfp4":
        acc_down, acc_up = acc_quant.quantize_tensor(acc_down, "mxfp4")
    return dict(d, q_down=acc_down, q_up=acc_up, kind=KINDS[kind])


def _skinny(cd, layers, flagged, s=0.5, x_shared=False):
    """sow_forward_skinny: flagged -- fp32 factors with cd | SOW_PARAM_F32 | SOW_ACC_NATIVE; else the factors pre-rounded, cd."""
    lib = _lib.load()
    code = CODE[cd] | (PF | NATIVE if flagged else 0)
    pdt = F32 if flagged else cd
    arr = (_lib.LayerArgs * len(layers))()
    ys, keep = [], []
    x0 = _dev(layers[0]["x"])
    for i, d in enumerate(layers):
        T, d_in = d["x"].shape
        r, d_out = d["B"].shape
        x = x0 if x_shared else _dev(d["x"])
        A, B, bias = _dev(d["A"], pdt), _dev(d["B"], pdt), _dev(d["bias"], pdt)
        y = torch.full((T, d_out), float("nan"), dtype=cd, device=DEV)
        q = {_lib.ACC_DENSE_FP8: lib.sow_forward_skinny_fp8_workspace_bytes, _lib.ACC_DENSE_FP4: lib.sow_forward_skinny_fp4_workspace_bytes}
        nws = (q[d["kind"]](T, d_in, d_out, r, code) if d["kind"] in q
               else lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, d["kind"], code))
        assert nws > 0, (T, d_in, d_out, r, d["kind"], hex(code))
        ws = _Ws(nws)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (E._ptr(t) for t in (x, A, B, d["q_down"], d["q_up"], bias, y))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, d["kind"], s
        a.workspace, a.workspace_bytes = ws.ptr(), ws.n
        ys.append(y), keep.append((x, A, B, bias, ws))
    _lib.check(lib.sow_forward_skinny(arr, len(layers), code, E._stream()), "sow_forward_skinny" + (" (flagged)" if flagged else ""))
    torch.cuda.synchronize()
    for k in keep:
        k[-1].check("skinny")
    return ys


@pytest.mark.parametrize("shape", [(160, 136), (512, 512)], ids=["160x136", "512x512"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_skinny_fp32_factors_equal_pre_rounded(dt, kind, shape):
    cd = DT[dt]
    d_in, d_out = shape
    for T in (1, 17, 32):
        for r in (8, 50):
            for bias in (True, False):
                d = _skinny_layer(cd, kind, T, d_in, d_out, r, bias)
                (got,), (want,) = _skinny(cd, [d], True), _skinny(cd, [d], False)
                _same(got, want, f"{dt} {kind} {shape} T={T} r={r} bias={bias}")
                assert bool(torch.isfinite(got.float()).all()) and float(got.float().abs().max()) > 0


@pytest.mark.parametrize("kind", ["dense", "mxfp4"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_skinny_qkv_in_one_call(dt, kind):
    cd = DT[dt]
    layers = [_skinny_layer(cd, kind, 17, 512, 512, r, i != 1, seed=20 + i) for i, r in enumerate((8, 50, 50))]
    for d in layers[1:]:
        d["x"] = layers[0]["x"]
    got, want = _skinny(cd, layers, True, x_shared=True), _skinny(cd, layers, False, x_shared=True)
    singles = [_skinny(cd, [d], True)[0] for d in layers]
    for i in range(3):
        _same(got[i], want[i], f"{dt} {kind} sibling {i}")
        _same(got[i], singles[i], f"{dt} {kind} sibling {i} against its call alone")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_skinny_nan_in_b_reaches_exactly_its_column(dt, kind):
    cd = DT[dt]
    T, d_in, d_out, r = 17, 160, 136, 8
    d = _skinny_layer(cd, kind, T, d_in, d_out, r, True)
    (clean,) = _skinny(cd, [d], True)
    j0, n0 = 5, 77
    d["B"] = d["B"].clone()
    d["B"][j0, n0] = float("nan")
    (got,), (want,) = _skinny(cd, [d], True), _skinny(cd, [d], False)
    assert bool(torch.isnan(got[:, n0]).all()), "the NaN of B[j0, n0] reaches every row of column n0"
    keep = torch.ones(d_out, dtype=torch.bool, device=DEV)
    keep[n0] = False
    _same(got[:, keep].contiguous(), clean[:, keep].contiguous(), "every other column is the clean run's")
    assert bool(torch.isnan(want[:, n0]).all())
    _same(got[:, keep].contiguous(), want[:, keep].contiguous(), "against the pre-rounded call")


# ---- 3. the module surface ----------------------------------------------------------------------------------------------------------
class _Net(nn.Module):
    """One layer (o_proj) or q / k / v siblings on one input, d -> d, biased, built in `cd` with a dense accumulator."""

    def __init__(self, d, r, cd, group, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.self_attn = nn.Module()
        self.names = ("q_proj", "k_proj", "v_proj") if group else ("o_proj",)
        self.master = []
        for nm in self.names:
            m = SoWLinear(d, d, bias=True, rank=r, init_method="normal", scale=0.5, device=DEV, dtype=cd)
            m.acc_downweight = nn.Parameter((torch.randn(d, d, generator=g) * 0.02).to(DEV, cd), requires_grad=False)
            self.master.append((_master((d, r), 0.05, cd, g), _master((r, d), 0.05, cd, g), _master((d,), 0.1, cd, g)))
            setattr(self.self_attn, nm, m)

    def layers(self):
        return [getattr(self.self_attn, nm) for nm in self.names]

    def set_master(self):
        """After master_factors: the fp32 values that are no numbers of the compute dtype."""
        with torch.no_grad():
            for m, (A, B, b) in zip(self.layers(), self.master):
                assert m.downscale_weights[0].dtype == F32 and m.upscale_weights[0].dtype == F32 and m.bias.dtype == F32
                m.downscale_weights[0].copy_(A), m.upscale_weights[0].copy_(B), m.bias.copy_(b)

    def forward(self, x):
        ys = [m(x) for m in self.layers()]
        return ys[0] if len(ys) == 1 else ys[0] + ys[1] * 0.5 - ys[2]


def _nets(d, r, cd, group, seed=5, quant=None):
    """(net, twin).  net: fp32 master factors over an accumulator of cd -- or, quant = "fp8_e4m3" / "mxfp4", over its codes.
    twin: the same factors over the fp32 copy of the accumulator (the existing SOW_PARAM_F32 path) -- or over the image W^ in cd."""
    import sow_amd
    net = _Net(d, r, cd, group, seed)
    twin = copy.deepcopy(net)
    if quant:
        assert quantize_accumulators(net, fmt=quant, strict=True) == len(net.names)
        twin = copy.deepcopy(net)
        assert dequantize_accumulators(twin) == len(twin.names)          # (while its factors are of cd: the image is of cd)
    for n in (net, twin):
        assert sow_amd.master_factors(n) == len(n.names)
        n.set_master()
    for m, t in zip(net.layers(), twin.layers()):
        if quant:
            assert m.acc_quantized() and m.acc_downweight.dtype in ops.CODES and t.acc_downweight.dtype == cd
        else:
            assert m.acc_downweight.dtype == cd, "master_factors leaves the accumulator alone"
            t.acc_downweight = nn.Parameter(t.acc_downweight.data.float(), requires_grad=False)
    if group:
        assert group_siblings(net) == 1 and group_siblings(twin) == 1
    return net, twin


def _train_step(net, x, dy, sink, cd):
    bucket = None
    if sink:
        bucket = FactorBucket(factor_parameters(net, biases=True))
        assert bucket.attach(net) == len(net.names)
        bucket.zero_grad()
    else:
        for p in net.parameters():
            p.grad = None
    xin = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=cd):
        y = net(xin)
    y.backward(dy)
    if bucket is not None:
        bucket.finalize()
    torch.cuda.synchronize()
    out = dict(y=y.detach(), dx=xin.grad)
    for i, m in enumerate(net.layers()):
        out[f"dA{i}"], out[f"dB{i}"], out[f"dbias{i}"] = (m.downscale_weights[0].grad, m.upscale_weights[0].grad, m.bias.grad)
    assert all(v is not None for v in out.values())
    assert out["y"].dtype == cd and out["dA0"].dtype == F32
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "bucket"])
@pytest.mark.parametrize("group", [False, True], ids=["single", "qkv"])
@pytest.mark.parametrize("T", [64, 8193])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_module_training_equals_the_fp32_accumulator_twin(dt, T, group, sink):
    cd, d, r = DT[dt], 264, 16
    net, twin = _nets(d, r, cd, group)
    g = torch.Generator().manual_seed(T)
    x, dy = torch.randn(T, d, generator=g).to(DEV, cd), torch.randn(T, d, generator=g).to(DEV, cd)
    got, want = _train_step(net, x, dy, sink, cd), _train_step(twin, x, dy, sink, cd)
    for k in want:
        _same(got[k], want[k], f"{k} against the twin with an fp32 accumulator")
    assert float(got["dx"].float().abs().max()) > 0 and all(m.acc_downweight.dtype == cd for m in net.layers())
    with torch.no_grad(), torch.autocast("cuda", dtype=cd):      # no-grad at T > 32: the existing forward, flagged
        _same(net(x), twin(x), "no-grad forward")


@pytest.mark.parametrize("group", [False, True], ids=["single", "qkv"])
@pytest.mark.parametrize("quant", ["fp8_e4m3", "mxfp4"])
def test_module_quantised_training_equals_the_image_twin(quant, group):
    cd, d, r, T = BF16, 288, 16, 64
    net, twin = _nets(d, r, cd, group, seed=7, quant=quant)
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(T, d, generator=g).to(DEV, cd), torch.randn(T, d, generator=g).to(DEV, cd)
    for sink in (False, True):
        got, want = _train_step(net, x, dy, sink, cd), _train_step(twin, x, dy, sink, cd)
        for k in want:
            _same(got[k], want[k], f"{quant} sink={sink}: {k} against the twin on the image")
    assert all(m.acc_quantized() for m in net.layers()), "autograd saves codes and scales: the layer stays quantised"


@pytest.mark.parametrize("T", [4, 17])
@pytest.mark.parametrize("quant", [None, "fp8_e4m3", "mxfp4"], ids=["native", "e4m3", "mxfp4"])
@pytest.mark.parametrize("group", [False, True], ids=["single", "qkv"])
def test_module_no_grad_generation_step_equals_the_cabi_skinny_call(monkeypatch, group, quant, T):
    cd, d, r = BF16, 288, 16
    net, _ = _nets(d, r, cd, group, seed=9, quant=quant)
    calls = []
    orig = ops.sow_forward_skinny
    monkeypatch.setattr(ops, "sow_forward_skinny", lambda layers: (calls.append(len(layers)), orig(layers))[1])
    x = torch.randn(T, d, generator=torch.Generator().manual_seed(2)).to(DEV, cd)
    with torch.no_grad(), torch.autocast("cuda", dtype=cd):
        ys = [m(x) for m in net.layers()]
    assert calls == [len(net.names)], f"one skinny call for the set, no other path: {calls}"
    for i, (m, y) in enumerate(zip(net.layers(), ys)):
        acc_down, acc_up = m._acc_pair()
        layer = dict(x=x.cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(), bias=m.bias.data.cpu(),
                     q_down=acc_down.data, q_up=acc_up if quant else None, kind=ops.acc_kind(acc_down, acc_up))
        assert layer["A"].dtype == F32 and y.dtype == cd
        (want,) = _skinny(cd, [layer], True, s=float(m.scale))
        _same(y, want, f"projection {i} against the C-ABI skinny call")
    # an fp32 input is cast once and takes the same route
    calls.clear()
    with torch.no_grad(), torch.autocast("cuda", dtype=cd):
        y32 = net.layers()[0](x.float())
    assert calls == [len(net.names)]
    _same(y32, ys[0], "fp32 input")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_accumulate_keeps_the_accumulator_dtype(dt):
    import sow_amd
    cd, d, r = DT[dt], 264, 16
    net, _ = _nets(d, r, cd, False, seed=11)
    (m,) = net.layers()
    m.virtual_rank = d                    # the dense-accumulator branch, as prepare_sow sets it up
    W0, A0, B0 = m.acc_downweight.data.clone(), m.downscale_weights[0].data.clone(), m.upscale_weights[0].data.clone()
    want = ops.gemm(A0.to(cd), B0.to(cd), out=W0.clone(), alpha=float(m.scale), beta=1.0)
    pA = m.downscale_weights[0]
    sow_amd.accumulate(net)
    assert m.acc_downweight.dtype == cd and tuple(m.acc_downweight.shape) == (d, d), "the accumulator keeps its dtype"
    _same(m.acc_downweight.data, want, "rn(W + s rn(A) rn(B)) from the existing gemm")
    assert not torch.equal(_bits(want), _bits(W0))
    assert m.downscale_weights[0] is pA and pA.dtype == F32 and m.upscale_weights[0].dtype == F32, "new factors in the factor dtype"
    assert bool((m.upscale_weights[0].data == 0).all()) and float(pA.data.abs().max()) > 0
    # a quantised layer keeps raising
    qnet, _ = _nets(288, r, cd, False, seed=12, quant="fp8_e4m3")
    with pytest.raises(RuntimeError, match="dequantize_accumulators"):
        qnet.layers()[0].accumulate()


def test_check_accumulator_forms():
    x = torch.zeros(4, 64, device=DEV, dtype=BF16)
    for adt in (F32, BF16):
        W = torch.zeros(64, 64, device=DEV, dtype=adt)
        assert ops.check_accumulator(x, 64, 64, W, None, param_dtype=F32) == (_lib.ACC_DENSE, 0)
        assert bool(ops._call_dtype(x, True, acc_down=W)[0] & NATIVE) == (adt == BF16)
    with pytest.raises(TypeError, match="dtype mismatch"):
        ops.check_accumulator(x, 64, 64, torch.zeros(64, 64, device=DEV, dtype=F16), None, param_dtype=F32)
    with pytest.raises(TypeError, match="dtype mismatch"):      # a low-rank accumulator of two dtypes
        ops.check_accumulator(x, 64, 64, torch.zeros(64, 8, device=DEV, dtype=BF16), torch.zeros(8, 64, device=DEV, dtype=F32),
                              param_dtype=F32)
    with pytest.raises(TypeError, match="dtype mismatch"):      # outside mixed precision nothing changes
        ops.check_accumulator(x, 64, 64, torch.zeros(64, 64, device=DEV, dtype=F32), None)
    codes, exps = acc_quant.quantize_tensor(torch.randn(64, 64, device=DEV).to(BF16))
    assert ops.check_accumulator(x, 64, 64, codes, exps, param_dtype=F32)[0] == _lib.ACC_DENSE_FP8


# ---- 4. HIP graph capture ------------------------------------------------------------------------------------------------------------
def test_graph_replay_module_forward_backward():
    """A layer's forward + backward under autocast at T = 64, captured on a side stream: the factor pack is part of the graph,
    so replays on x, dY and the fp32 factors changed in place equal the eager twins; the accumulator is read where it lies."""
    cd, T, d, r = BF16, 64, 264, 16
    net, twin = _nets(d, r, cd, False, seed=31)
    (m,), (mt,) = net.layers(), twin.layers()
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(T, d, generator=g).to(cd) * s for s in (1.0, 0.5)]
    dys = [torch.randn(T, d, generator=g).to(cd) for _ in (0, 1)]
    sets = [net.master[0], (_master((d, r), 0.05, cd, g), _master((r, d), 0.05, cd, g), _master((d,), 0.1, cd, g))]
    params = (m.downscale_weights[0], m.upscale_weights[0], m.bias)
    b = GR.Bound("acc_native_module")
    ar, ar32 = b.arena(cd), b.arena(F32)
    x, dy = b.input(ar, (xs[0], xs[1])), b.input(ar, (dys[0], dys[1]))
    for i, p in enumerate(params):
        b.extra(None, p.data, (sets[0][i], sets[1][i]))
    outs = {k: b.output(ar, k, s) for k, s in (("y", (T, d)), ("dx", (T, d)))}
    outs.update({k: b.output(ar32, k, s) for k, s in (("dA", (d, r)), ("dB", (r, d)), ("dbias", (d,)))})

    def call(rc):
        for p in params:
            p.grad = None
        xin = x.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=cd):
            yy = net(xin)
        yy.backward(dy)
        for k, v in zip(("y", "dx", "dA", "dB", "dbias"), (yy.detach(), xin.grad, *(p.grad for p in params))):
            outs[k].copy_(v)

    b.call = call

    def check(k, out):
        with torch.no_grad():
            for dst, src in zip((mt.downscale_weights[0], mt.upscale_weights[0], mt.bias), sets[k]):
                dst.copy_(src)
        want = _train_step(twin, xs[k].to(DEV), dys[k].to(DEV), False, cd)
        for key, wk in (("y", "y"), ("dx", "dx"), ("dA", "dA0"), ("dB", "dB0"), ("dbias", "dbias0")):
            _same(out[key], want[wk].cpu(), f"replay on input set {k + 1}: {key} against the eager twin")

    b.check = check
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "pack_params_kernel"), sorted(set(trace))
