"""-m gpu: the generation-sized forward (sow_forward_skinny, skinny_fwd.hip) through the C ABI, element by element against
float64, and the module surface that dispatches to it (SoWLinear / SiblingGroup under torch.no_grad() at T <= 32).

The contract (include/sow_amd.h):  h = rn(scale * x A)  (fp32 sum, rounded once to the compute dtype, never stored),
y = rn(x W_acc + h B + bias)  (one fp32 sum, ONE rounding).  The float64 reference is built from the same bf16 / f16
operands with h rounded as the contract says; every element of y is held to numerics.bound with one output rounding and
the fp32 accumulation floor of its d_in + max(r, 64) terms -- the comparator test_gpu_elementwise.py applies to its dense
cases, no other tolerance.  Buffers are owned by the test as there: NaN neighbours around every input, sentinel guards
around every output, y and the workspace filled with 0xFF bytes before each of three runs that must agree bit for bit.

Shapes: (264, 520), (520, 264) and (1032, 72) leave the last K-slab and the last 64-column range partial (264 = 2 x 128 + 8:
a slab of one k-group; 520 = 8 x 64 + 8; 72 = 64 + 8; 1032 = 8 x 128 + 8); T = 16 / 17 sit on both sides of the second row
tile; r = 2, 8, 50, 64 take one to four fragment columns of x A, partial and full.
"""
import copy

import pytest
import torch
import torch.nn as nn

import fuzz_plan as FP
import test_gpu_elementwise as E
import value_plan as VP
from numerics import bound, check_bound, fp32_floor, rne, to64
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DT = {"bf16": BF16, "f16": F16}
ERR_DTYPE, ERR_UNSUPPORTED = -3, -6
WORST = {}

# (dtype, T, d_in, d_out, r, bias, scale, accumulator): a seeded draw (random.Random(20261017)) from
# T {1, 3, 16, 17, 32} x shape {(264, 520), (520, 264), (1032, 72)} x r {2, 8, 50, 64} x bias x scale {1, 0.25} x
# {dense, none} x {bf16, f16} that holds every (T, shape) pair and every (r, accumulator, dtype) triple at least once
CASES = [
    ('f16', 1, 264, 520, 8, True, 0.25, 'none'),
    ('f16', 1, 520, 264, 64, False, 1.0, 'dense'),
    ('bf16', 1, 1032, 72, 50, False, 1.0, 'none'),
    ('bf16', 3, 264, 520, 2, True, 0.25, 'dense'),
    ('f16', 3, 520, 264, 64, False, 1.0, 'dense'),
    ('f16', 3, 1032, 72, 64, False, 0.25, 'dense'),
    ('f16', 16, 264, 520, 8, False, 0.25, 'dense'),
    ('bf16', 16, 520, 264, 50, False, 1.0, 'dense'),
    ('f16', 16, 1032, 72, 8, False, 1.0, 'dense'),
    ('f16', 17, 264, 520, 8, True, 1.0, 'dense'),
    ('bf16', 17, 520, 264, 64, True, 1.0, 'dense'),
    ('f16', 17, 1032, 72, 64, True, 1.0, 'dense'),
    ('f16', 32, 264, 520, 2, True, 1.0, 'none'),
    ('f16', 32, 520, 264, 2, True, 1.0, 'dense'),
    ('bf16', 32, 1032, 72, 2, False, 0.25, 'dense'),
    ('bf16', 32, 520, 264, 2, False, 0.25, 'dense'),
    ('f16', 17, 520, 264, 2, False, 1.0, 'dense'),
    ('bf16', 3, 264, 520, 2, True, 0.25, 'none'),
    ('f16', 1, 1032, 72, 2, True, 0.25, 'none'),
    ('bf16', 17, 520, 264, 8, True, 1.0, 'dense'),
    ('f16', 17, 264, 520, 8, False, 1.0, 'dense'),
    ('bf16', 17, 520, 264, 8, False, 0.25, 'none'),
    ('f16', 17, 1032, 72, 8, False, 0.25, 'none'),
    ('bf16', 17, 1032, 72, 50, True, 1.0, 'dense'),
    ('f16', 16, 520, 264, 50, False, 0.25, 'dense'),
    ('bf16', 32, 520, 264, 50, False, 1.0, 'none'),
    ('f16', 16, 1032, 72, 50, True, 0.25, 'none'),
    ('bf16', 3, 520, 264, 64, True, 0.25, 'dense'),
    ('f16', 17, 520, 264, 64, False, 0.25, 'dense'),
    ('bf16', 17, 264, 520, 64, False, 1.0, 'none'),
    ('f16', 32, 264, 520, 64, False, 0.25, 'none'),
    ('f16', 17, 520, 264, 8, False, 0.25, 'none'),
    ('f16', 17, 520, 264, 2, False, 0.25, 'none'),
    ('f16', 17, 520, 264, 2, True, 0.25, 'none'),
    ('bf16', 17, 264, 520, 64, True, 0.25, 'dense'),
    ('f16', 32, 264, 520, 2, True, 0.25, 'none'),
    ('f16', 1, 520, 264, 2, True, 1.0, 'dense'),
    ('f16', 17, 264, 520, 8, False, 0.25, 'dense'),
    ('bf16', 16, 520, 264, 8, False, 0.25, 'dense'),
    ('bf16', 32, 264, 520, 64, False, 0.25, 'dense'),
]


def _id(c):
    return "-".join(str(v) for v in c)


def _gauss(dtype, T, d_in, d_out, r, bias, acc, seed=0):
    """Gaussian operands of one layer, rounded to `dtype` (CPU tensors): x ~ N(0, 1), factors 0.05, accumulator 0.02."""
    g = torch.Generator().manual_seed(5000 + seed + 7 * T + 3 * r + d_in)
    rnd = lambda *shape, std=1.0: (torch.randn(*shape, generator=g) * std).to(dtype)   # noqa: E731
    return dict(x=rnd(T, d_in), A=rnd(d_in, r, std=0.05), B=rnd(r, d_out, std=0.05),
                bias=rnd(d_out, std=0.1) if bias else None, W=rnd(d_in, d_out, std=0.02) if acc == "dense" else None)


def _call(arr, n, dtype):
    return _lib.load().sow_forward_skinny(arr, n, E._dt(dtype), E._stream())


def _run(dtype, layers, x_shared=False, runs=(0xFF, 0x00, 0xFF), what="skinny"):
    """One sow_forward_skinny call over `layers` (dicts of CPU operands + scale "s"), repeated on poisoned, zeroed and
    poisoned memory: the runs must agree bit for bit and leave every guard intact.  Returns the y of the first run (CPU).
    x_shared: every layer reads the first layer's x buffer."""
    lib = _lib.load()
    ar = E.Arena(dtype)
    arr = (_lib.LayerArgs * len(layers))()
    ys, keep = [], []
    x0 = None
    for i, d in enumerate(layers):
        x = x0 if (x_shared and x0 is not None) else ar.input(d["x"])
        x0 = x0 if x0 is not None else x
        A, B, bias, W = (ar.input(d[k]) for k in ("A", "B", "bias", "W"))
        T, d_in = d["x"].shape
        r, d_out = d["B"].shape
        kind = _lib.ACC_DENSE if W is not None else _lib.ACC_NONE
        y = ar.output((T, d_out))
        nws = lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, E._dt(dtype))
        assert nws > 0, (T, d_in, d_out, r, kind)
        ws = ar.workspace(nws)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.bias, a.y = (E._ptr(t) for t in (x, A, B, W, bias, y))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, d["s"]
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        ys.append(y)
        keep.append((x, A, B, bias, W, ws))
    outs = []
    for byte in runs:
        ar.fill(byte)
        _lib.check(_call(arr, len(layers), dtype), "sow_forward_skinny")
        ar.check_guards(f"{what} run {len(outs)}")
        outs.append([y.clone() for y in ys])
    for k in range(1, len(outs)):
        for i, (a, b) in enumerate(zip(outs[0], outs[k])):
            assert torch.equal(E._bits(a), E._bits(b)), f"{what}: y of layer {i} differs between run 0 and run {k}"
    return [y.cpu() for y in outs[0]]


def _reference(dtype, d):
    """(y_ref, y_sq, n_y) in float64 from the operands of one layer: h rounded once to the compute dtype, as the contract
    says; y_sq = the sum of the squared terms of y's one fp32 sum, n_y its length as test_gpu_elementwise counts it."""
    q = {k: to64(v) for k, v in d.items() if isinstance(v, torch.Tensor)}
    x, A, B = q["x"], q["A"], q["B"]
    h = rne(d["s"] * (x @ A), dtype)
    y = h @ B
    sq = (h * h) @ (B * B)
    if "W" in q:
        y = y + x @ q["W"]
        sq = sq + (x * x) @ (q["W"] * q["W"])
    if "bias" in q:
        y = y + q["bias"]
    return y, sq, x.shape[1] + max(A.shape[1], 64)


def _check(name, dtype, d, y):
    y_ref, y_sq, n_y = _reference(dtype, d)
    st = check_bound(y, y_ref, bound(y_ref, dtype, fp32_floor(y_sq, n_y)), name=f"{name}: y")
    WORST[name] = st["worst"]
    print(f"{name}: worst err / bound = {st['worst']:.3f}")
    return st


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_elementwise_against_fp64(c):
    dt, T, d_in, d_out, r, bias, s, acc = c
    dtype = DT[dt]
    d = dict(_gauss(dtype, T, d_in, d_out, r, bias, acc), s=s)
    (y,) = _run(dtype, [d], what=_id(c))
    _check(_id(c), dtype, d, y)


def test_long_k_slabs():
    """The shapes above all plan 128-deep K-slabs (one k-step per wave).  3592 -> 8200 has 129 column ranges, so the plan
    takes four slabs of 1024, 1024, 1024 and 520: eight k-steps per wave (the request-ahead ring of four refilled and
    drained, a wave with a partial last round), and at T = 32 the 66 KB x slab that needs the raised LDS limit."""
    lib = _lib.load()
    # the planned slab count, read off the workspace query: 256 + S * T * d_out * 4 (256-aligned) + S * T * 64 * 4
    assert lib.sow_forward_skinny_workspace_bytes(32, 3592, 8200, 50, _lib.ACC_DENSE, _lib.BF16) == 256 + 4 * 32 * (8200 + 64) * 4
    d = dict(_gauss(BF16, 32, 3592, 8200, 50, True, "dense", seed=40), s=0.5)
    (y,) = _run(BF16, [d], what="long slabs")
    _check("long_slabs", BF16, d, y)


# ---- exact operands ---------------------------------------------------------------------------------------------------
EXACT = [("bf16", 17, 264, 520, 50, True, 0.5, "dense"), ("f16", 32, 520, 264, 8, True, 0.25, "dense"),
         ("bf16", 3, 1032, 72, 64, False, 1.0, "none"), ("f16", 16, 264, 520, 2, True, 0.5, "dense")]


def _exact_operands(c):
    """value_plan's exact operands of a case, with the proof this kernel needs, in float64 on the CPU: h representable in the
    compute dtype, and every sum the kernel forms -- x A, and x W + h B + bias in one accumulator -- made of multiples of
    one unit with sum |terms| below 2^24 units, so that every partial sum (any slab, wave or k order) is exact in fp32."""
    dt, T, d_in, d_out, r, bias, s, acc = c
    lc = FP.Layer(name="skinny_exact_" + _id(c), dtype=dt, T=T, d_in=d_in, d_out=d_out, r=r, acc=None if acc == "none" else acc,
                  bias=bias, s=s, save_h=False, seed=11)
    err = None
    for level in range(5):
        d = VP.exact_layer(lc, level)
        try:
            f = VP.prove_layer(lc, d)
            break
        except VP.NotExact as e:
            err = e
    else:
        raise err
    dtype = DT[dt]
    q = {k: to64(v) for k, v in d.items() if v is not None}
    x, A, B = q["x"], q["A"], q["B"]
    h = s * (x @ A)
    assert bool((rne(h, dtype) == h).all()), "h is not representable in the compute dtype"
    assert float((x.abs() @ A.abs()).max()) / (VP.lsb(x) * VP.lsb(A)) < VP.EXACT_UNITS, "x A: a partial sum may be inexact"
    units = [VP.lsb(h) * VP.lsb(B)]
    total = h.abs() @ B.abs()
    y = h @ B
    if "W" in q:
        units.append(VP.lsb(x) * VP.lsb(q["W"]))
        total = total + x.abs() @ q["W"].abs()
        y = y + x @ q["W"]
    if "bias" in q:
        units.append(VP.lsb(q["bias"]))
        total = total + q["bias"].abs()
        y = y + q["bias"]
    assert float(total.max()) / min(units) < VP.EXACT_UNITS, "y: a partial sum may be inexact"
    assert float((y != 0).double().mean()) >= 0.5, "exactness bought with emptiness"
    assert bool((y == f["y"]).all())
    ops = dict(x=d["x"].to(dtype), A=d["A"].to(dtype), B=d["B"].to(dtype), bias=None if d.get("bias") is None else d["bias"].to(dtype),
               W=d["W"].to(dtype) if "W" in d else None, s=s)
    return ops, y


@pytest.mark.parametrize("c", EXACT, ids=_id)
def test_exact_operands_bit_for_bit(c):
    dtype = DT[c[0]]
    d, y64 = _exact_operands(c)
    (y,) = _run(dtype, [d], what="exact " + _id(c))
    want = rne(y64, dtype)
    got = to64(y)
    bad = got != want
    assert not bad.any(), (f"{int(bad.sum())} of {bad.numel()} elements differ from the float64 result rounded once; first at "
                           f"{tuple(int(v) for v in torch.nonzero(bad)[0])}: {float(got[bad][0])} vs {float(want[bad][0])}")


def test_exact_group_equals_single_calls():
    """The exact operands of two bf16 cases in one grouped call: bit for bit the single calls (which the test above ties to
    float64)."""
    cases = [c for c in EXACT if c[0] == "bf16"]
    ds = [_exact_operands(c)[0] for c in cases]
    grouped = _run(BF16, ds, what="exact group")
    for c, d, yg in zip(cases, ds, grouped):
        (ys,) = _run(BF16, [d], runs=(0xFF,), what="exact single " + _id(c))
        assert torch.equal(E._bits(yg), E._bits(ys)), _id(c)


# ---- rows, determinism, groups ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,k", [("bf16", 0), ("bf16", 263), ("f16", 130)])
def test_rows_are_independent(dt, k):
    """T = 3 with a NaN in x[1, k]: row 1 of y is NaN, rows 0 and 2 keep their bits.  A pad row read from memory instead of
    generated as zeros, or a tile that mixes tokens, fails here (and the NaN neighbours of every input in all tests)."""
    dtype = DT[dt]
    d = dict(_gauss(dtype, 3, 264, 520, 50, True, "dense", seed=3), s=0.5)
    (clean,) = _run(dtype, [d], runs=(0xFF,), what="rows clean")
    p = dict(d, x=d["x"].clone())
    p["x"][1, k] = float("nan")
    (poisoned,) = _run(dtype, [p], runs=(0xFF,), what="rows poisoned")
    assert bool(torch.isnan(poisoned[1]).all()), "row 1 must be NaN in every column"
    for t in (0, 2):
        assert torch.equal(E._bits(poisoned[t]), E._bits(clean[t])), f"row {t} changed"
    _check(f"rows_{dt}_{k}", dtype, d, clean)


def test_three_calls_on_repoisoned_memory_are_identical():
    d = dict(_gauss(BF16, 32, 1032, 72, 50, True, "dense", seed=5), s=1.0)
    (y,) = _run(BF16, [d], runs=(0xFF, 0xFF, 0xFF), what="determinism")   # _run asserts the three runs bit-identical
    _check("determinism", BF16, d, y)


def test_groups_equal_single_calls():
    # three siblings on ONE x buffer: 512 -> {512, 256, 256}, r = 50
    g = torch.Generator().manual_seed(9)
    x = torch.randn(5, 512, generator=g).to(BF16)
    sibs = []
    for i, d_out in enumerate((512, 256, 256)):
        d = dict(_gauss(BF16, 5, 512, d_out, 50, i == 1, "dense", seed=20 + i), s=0.5)
        d["x"] = x
        sibs.append(d)
    grouped = _run(BF16, sibs, x_shared=True, what="qkv group")
    for i, (d, yg) in enumerate(zip(sibs, grouped)):
        (ys,) = _run(BF16, [d], runs=(0xFF,), what=f"qkv single {i}")
        assert torch.equal(E._bits(yg), E._bits(ys)), f"sibling {i}"
        _check(f"qkv_{i}", BF16, d, yg)
    # two layers on different inputs with different token counts (4 and 32), one with an accumulator and one without
    pair = [dict(_gauss(F16, 4, 264, 520, 8, True, "dense", seed=30), s=0.25),
            dict(_gauss(F16, 32, 520, 264, 64, False, "none", seed=31), s=1.0)]
    grouped = _run(F16, pair, what="mixed group")
    for i, (d, yg) in enumerate(zip(pair, grouped)):
        (ys,) = _run(F16, [d], runs=(0xFF,), what=f"mixed single {i}")
        assert torch.equal(E._bits(yg), E._bits(ys)), f"layer {i}"
        _check(f"mixed_{i}", F16, d, yg)


# ---- refusals -----------------------------------------------------------------------------------------------------------
REFUSALS = [("T=33", dict(T=33), 0, ERR_UNSUPPORTED, {}), ("lowrank", dict(kind=_lib.ACC_LOWRANK), 0, ERR_UNSUPPORTED, {}),
            ("r=66", dict(r=66), 0, ERR_UNSUPPORTED, {}), ("d_out=523", dict(d_out=523), 0, ERR_UNSUPPORTED, {}),
            ("fp32", {}, None, ERR_DTYPE, {}), ("param_f32", {}, _lib.PARAM_F32, ERR_UNSUPPORTED, {}),
            ("NO_SKINNY", {}, 0, ERR_UNSUPPORTED, dict(NO_SKINNY=1))]


@pytest.mark.parametrize("name,kw,flag,code,switches", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_touch_nothing(name, kw, flag, code, switches):
    """Real buffers large enough for the refused shape; y and the workspace hold 0xFF bytes before and after."""
    T, d_in, d_out, r, kind = kw.get("T", 4), 264, kw.get("d_out", 520), kw.get("r", 8), kw.get("kind", _lib.ACC_DENSE)
    z = lambda *s: torch.zeros(*s, dtype=BF16, device=DEV)   # noqa: E731
    x, A, B, W, up, bias = z(T, d_in), z(d_in, r), z(r, d_out), z(d_in, d_out), z(d_in, d_out), z(d_out)
    y = torch.empty(T, d_out, dtype=BF16, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    y.view(torch.int16).fill_(-1)
    ws.fill_(0xFF)
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (t.data_ptr() for t in (x, A, B, W, up, bias, y))
    a.T, a.d_in, a.d_out, a.r_live, a.r_acc, a.acc_kind, a.scale = T, d_in, d_out, r, d_out, kind, 1.0
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    dtype = _lib.F32 if flag is None else (_lib.BF16 | flag)
    with _lib.switch(**switches):
        rc = _lib.load().sow_forward_skinny(arr, 1, dtype, E._stream())
    torch.cuda.synchronize()
    assert rc == code
    assert bool((y.view(torch.int16) == -1).all()), "y was written by a refused call"
    assert bool((ws == 0xFF).all()), "the workspace was written by a refused call"


# ---- module surface -------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    """A decoder block's seven projections under their HF names; every projection's (module, input, output) is recorded."""

    def __init__(self, d, inter, r, dtype):
        super().__init__()
        from sow_amd import SoWLinear
        mk = lambda i, o: SoWLinear(i, o, bias=False, rank=r, init_method="normal", scale=0.5, device=DEV, dtype=dtype)   # noqa: E731
        self.self_attn, self.mlp = nn.Module(), nn.Module()
        a, m = self.self_attn, self.mlp
        a.q_proj, a.k_proj, a.v_proj, a.o_proj = mk(d, d), mk(d, d), mk(d, d), mk(d, d)
        m.gate_proj, m.up_proj, m.down_proj = mk(d, inter), mk(d, inter), mk(inter, d)

    def forward(self, x, rec):
        a, m = self.self_attn, self.mlp
        q, k, v = a.q_proj(x), a.k_proj(x), a.v_proj(x)
        t = torch.tanh(q) + k * 0.5 + v
        o = a.o_proj(t)
        h = x + o
        g, u = m.gate_proj(h), m.up_proj(h)
        z = torch.tanh(g) * u * 4
        dn = m.down_proj(z)
        rec += [(a.q_proj, x, q), (a.k_proj, x, k), (a.v_proj, x, v), (a.o_proj, t, o), (m.gate_proj, h, g), (m.up_proj, h, u),
                (m.down_proj, z, dn)]
        return h + dn


class _Stack(nn.Module):
    def __init__(self, d=512, inter=1376, r=50, dtype=BF16, blocks=2):
        super().__init__()
        self.layers = nn.ModuleList([_Block(d, inter, r, dtype) for _ in range(blocks)])

    def forward(self, x, rec):
        for b in self.layers:
            x = b(x, rec)
        return x


def _stack():
    from sow_amd import SoWLinear, group_siblings
    torch.manual_seed(21)
    net = _Stack()
    for m in net.modules():
        if isinstance(m, SoWLinear):
            nn.init.normal_(m.upscale_weights[0], std=0.05)
            acc = torch.randn(m.in_features, m.out_features, device=DEV, dtype=BF16) * 0.02
            m.acc_downweight = nn.Parameter(acc, requires_grad=False)      # a dense ("keep") accumulator
    assert group_siblings(net) == 4
    return net


def _count_skinny(monkeypatch):
    from sow_amd import ops
    calls = []
    orig = ops.sow_forward_skinny
    monkeypatch.setattr(ops, "sow_forward_skinny", lambda layers: (calls.append(len(layers)), orig(layers))[1])
    return calls


def _check_projections(rec, dtype, tag):
    for i, (m, xin, out) in enumerate(rec):
        d = dict(x=xin.reshape(-1, xin.shape[-1]).cpu(), A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(),
                 W=m.acc_downweight.data.cpu(), s=float(m.scale))
        assert all(t.dtype == dtype for t in (d["x"], d["A"], d["B"], d["W"], out))
        _check(f"{tag}_proj{i}", dtype, d, out.reshape(-1, out.shape[-1]).cpu())


def test_module_no_grad_generation_step(monkeypatch):
    net = _stack()
    calls = _count_skinny(monkeypatch)
    x = torch.randn(4, 1, 512, generator=torch.Generator().manual_seed(2)).to(DEV, BF16)
    rec = []
    with torch.no_grad():
        out = net(x, rec)
    assert out.shape == (4, 1, 512) and len(rec) == 14
    # per block: q / k / v in one call, o, gate / up in one call, down
    assert calls == [3, 1, 2, 1, 3, 1, 2, 1], calls
    _check_projections(rec, BF16, "module_bf16")
    # grad enabled: the training path, no skinny call
    del calls[:]
    out = net(x.clone().requires_grad_(True), [])
    assert calls == [] and out.requires_grad
    # T = 64 under no_grad: past the bound, no skinny call
    with torch.no_grad():
        net(torch.randn(64, 1, 512, device=DEV, dtype=BF16), [])
    assert calls == []
    # the library's switch: the module falls back to the existing path and still answers
    with _lib.switch(NO_SKINNY=1), torch.no_grad():
        rec2 = []
        net(x, rec2)
    assert calls == [3, 1, 2, 1, 3, 1, 2, 1]      # asked, refused (None), existing path taken
    for (_, _, a), (_, _, b) in zip(rec, rec2):
        assert a.shape == b.shape and bool(torch.isfinite(b).all())


def test_module_half_copy_generation_step(monkeypatch):
    """The reference's eval sequence: .half() and .eval(), then T = batch x beams rows per step."""
    from sow_amd import group_siblings
    net = copy.deepcopy(_stack()).half().eval()
    group_siblings(net)      # (deepcopy keeps the groups; re-installing them is harmless)
    calls = _count_skinny(monkeypatch)
    x = torch.randn(4, 1, 512, generator=torch.Generator().manual_seed(4)).to(DEV, F16)
    rec = []
    with torch.no_grad():
        net(x, rec)
    assert calls == [3, 1, 2, 1, 3, 1, 2, 1], calls
    _check_projections(rec, F16, "module_f16")


def test_zz_report_worst_ratios():
    for k, v in sorted(WORST.items(), key=lambda kv: -kv[1])[:10]:
        print(f"{k}: worst err / bound {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
