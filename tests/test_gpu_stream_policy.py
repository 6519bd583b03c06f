"""-m gpu: the saved projection (h_save / dh) of the chain kernel written as whole streaming rows through an LDS image, and
the cache-policy switches of the chain and row-owner weight-gradient kernels (NT_LOAD, TN_NO_NT_LOAD), and the value-neutral
launch-shape switches (NO_PERSIST, NO_PAIR_FLUSH, NO_PARK16, NO_NT_STORE).

None of them touches a value: every output, saved projection and workspace byte must equal, bit for bit, what the same call
leaves with NO_H_ROWS (the 8-byte pieces written before) and with NT_LOAD streaming every X; h_save and dh are also held
element by element to the float64 reference (tests/numerics.py: check_h_save).  Shapes are the smallest at which
the hand-off can go wrong: three blocks (T = 192), a ragged last block whose rows past T must stay unwritten (T = 200), more
blocks than resident workgroups (T = 64 * 513 + 8: a workgroup runs two blocks and reuses the ring slot of the image), one
stage (64 -> 64), a partial last stage (d_in = 72), no free column (r = 64), the 1.0 of column 63 with zeros in r..62
(r = 50), both park forms (bias / beta make the fp32 one), a 3-layer group whose members share one launch, a 4-layer group
whose 4 x 130 blocks exceed the 512 resident workgroups (the persistent loop crosses layer boundaries; NO_PERSIST launches one
workgroup per block) and a 4-sibling shared-input set through chain2_shared."""
import pytest
import torch

from numerics import UNIT_ROUNDOFF, accumulation_term, check_h_save, to64
from sow_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
PARENT = dict(NO_H_ROWS=1)                                  # h_save / dh as 8-byte pieces per lane
NEW = dict(NO_H_ROWS=0, NT_LOAD=0, TN_NO_NT_LOAD=0)
# value-neutral launch-shape switches: one workgroup per block, one 64-column slice per flush, fp32 park tiles, cached Y stores
NEUTRAL = [(n, {n: 1}) for n in ("NO_PERSIST", "NO_PAIR_FLUSH", "NO_PARK16", "NO_NT_STORE")]
TAIL = 64                                                   # guard rows past T in every output buffer
SCALE = 0.75


class Layer:
    """One layer's operands, NaN-filled outputs with TAIL guard rows, and a 0xFF-filled workspace."""

    def __init__(self, gen, T, d_in, d_out, r, dtype, variant, x=None, dxbuf=None):
        def rnd(*shape, s=1.0):
            return (torch.randn(*shape, generator=gen, device=DEV) * s).to(dtype)
        self.T, self.d_in, self.d_out, self.r, self.dtype = T, d_in, d_out, r, dtype
        self.x, self.dy = (rnd(T, d_in) if x is None else x), rnd(T, d_out)   # x / dxbuf given: a sibling of a shared-input set
        self.A, self.B = rnd(d_in, r, s=0.05), rnd(r, d_out, s=0.05)
        self.bias = rnd(d_out) if variant == "bias" else None
        self.acc = (rnd(d_in, 8, s=0.05), rnd(8, d_out, s=0.05)) if variant == "beta" else (None, None)
        self.ybuf = torch.empty((T + TAIL) * d_out, dtype=dtype, device=DEV)
        self.hbuf = torch.empty((T + TAIL) * 64, dtype=dtype, device=DEV)
        self.dxbuf = torch.empty((T + TAIL) * d_in, dtype=dtype, device=DEV) if dxbuf is None else dxbuf
        self.dA, self.dB = torch.zeros_like(self.A), torch.zeros_like(self.B)
        kind = _lib.ACC_LOWRANK if variant == "beta" else _lib.ACC_NONE
        nws = ops.workspace_bytes(T, d_in, d_out, r, 8 if variant == "beta" else 0, kind, dtype)
        raw = torch.empty(nws + 512, dtype=torch.uint8, device=DEV)
        off = (-raw.data_ptr()) % 256                       # the library aligns the workspace to 256 bytes: dh sits first
        self.ws = raw[off:off + nws + 255]
        self.call = ops.LayerCall(self.x, self.A, self.B, acc_down=self.acc[0], acc_up=self.acc[1], bias=self.bias, scale=SCALE,
                                  y=self.ybuf[:T * d_out].view(T, d_out), h=self.hbuf[:T * 64], dy2=self.dy,
                                  dx=self.dxbuf[:T * d_in].view(T, d_in), out=(self.dA, self.dB, None), workspace=self.ws)

    def poison(self):
        for b in (self.ybuf, self.hbuf, self.dxbuf):
            b.view(torch.int16).fill_(-1)                   # 0xFFFF: NaN in bf16 and f16
        self.ws.fill_(0xFF)

    def snapshot(self):
        return [b.view(torch.int16).clone() for b in (self.ybuf, self.hbuf, self.dxbuf)] + [self.ws.clone()]

    def dh(self):
        return self.ws[:self.T * 128].view(self.dtype).view(self.T, 64)


def run(layers, switches, phases=_lib.BWD_DATA, shared=False):
    grp = (ops.SharedInputGroup if shared else ops.LayerGroup)([L.call for L in layers])
    for L in layers:
        L.poison()
    with _lib.switch(**switches):
        fwd = grp.forward()
        bwd = grp.backward(phases)
    if shared:
        assert fwd and bwd, "the shared-input kernels did not admit the set"
    torch.cuda.synchronize()
    return [L.snapshot() for L in layers]


def check(layers, tag, shared=False):
    new = run(layers, NEW, shared=shared)
    # rows past T keep the NaN pattern; so does the workspace behind dh where no short-T split has its partials there
    for L in layers:
        T = L.T
        for name, buf, width in (("y", L.ybuf, L.d_out), ("h_save", L.hbuf, 64), ("dX", L.dxbuf, L.d_in)):
            assert (buf.view(torch.int16)[T * width:] == -1).all(), f"{tag}: {name} written past row T"
            assert not torch.isnan(buf[:T * width]).any(), f"{tag}: {name} has unwritten elements below row T"
        nst_nsl = (L.d_in + 63) // 64 + (L.d_out + 63) // 64
        if (T > 8192 or nst_nsl < 24) and L.acc[0] is None:
            assert (L.ws[T * 128:T * 128 + TAIL * 128] == 0xFF).all(), f"{tag}: dh written past row T"
    # float64: h_save = RNE(s x A), dh = RNE(s dY B^T); zeros in r..62, 1.0 in column 63 when it is free
    u32 = UNIT_ROUNDOFF[torch.float32]
    for L in layers:
        x, dy, A, B = to64(L.x), to64(L.dy), to64(L.A), to64(L.B)
        acc = accumulation_term(SCALE * SCALE * ((x * x) @ (A * A)), u32, L.d_in)
        check_h_save(L.hbuf[:L.T * 64], SCALE * (x @ A), L.r, L.dtype, acc=acc, name=f"{tag}: h_save")
        acc = accumulation_term(SCALE * SCALE * ((dy * dy) @ (B * B).t()), u32, L.d_out)
        check_h_save(L.dh(), SCALE * (dy @ B.t()), L.r, L.dtype, acc=acc, name=f"{tag}: dh")
    # bit for bit what the parent's behaviour leaves, and what NT_LOAD's streaming X leaves
    for name, sw in [("parent switches", PARENT), ("NT_LOAD", dict(NT_LOAD=1))] + NEUTRAL:
        other = run(layers, sw, shared=shared)
        for li, (a, b) in enumerate(zip(new, other)):
            for what, u, v in zip(("y", "h_save", "dX", "workspace (dh)"), a, b):
                assert torch.equal(u, v), f"{tag}: {what} of layer {li} differs from the run with {name}"


SHAPES = [(64, 64, 8), (512, 1376, 50), (1376, 512, 50), (128, 192, 64), (72, 64, 8)]
CASES = [(192, s, "plain") for s in SHAPES] + [(200, s, v) for s in SHAPES for v in ("plain", "bias", "beta")]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("T,shape,variant", CASES, ids=[f"T{t}-{s[0]}x{s[1]}r{s[2]}-{v}" for t, s, v in CASES])
def test_single_layer(T, shape, variant, dtype):
    gen = torch.Generator(device=DEV).manual_seed(1000 + T + shape[0])
    check([Layer(gen, T, *shape, dtype, variant)], f"T={T} {shape} {variant}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_more_blocks_than_resident_workgroups(dtype):
    gen = torch.Generator(device=DEV).manual_seed(7)
    check([Layer(gen, 64 * 513 + 8, 64, 64, 8, dtype, "plain")], "T=64*513+8 64->64")


@pytest.mark.parametrize("variant", ["plain", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_three_layers_in_one_launch(dtype, variant):
    """T > 8192: the three layers share one persistent grid (130 blocks each), ranks 8, 64 and 50 side by side."""
    gen = torch.Generator(device=DEV).manual_seed(11)
    T = 64 * 129 + 8
    check([Layer(gen, T, di, do, r, dtype, variant) for di, do, r in ((64, 64, 8), (64, 192, 64), (72, 64, 50))], f"group {variant}")


GROUP4 = ((64, 64, 8), (64, 192, 64), (72, 64, 50), (128, 64, 16))


@pytest.mark.parametrize("variant", ["plain", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_four_layers_cross_the_resident_grid(dtype, variant):
    """T = 8257: 4 x 130 = 520 blocks on 512 resident workgroups -- the persistent loop of a workgroup crosses a layer
    boundary; NO_PERSIST launches the 520 blocks.  `plain` takes the bf16 park (NO_PARK16 switches it off), `bias` the fp32 one."""
    gen = torch.Generator(device=DEV).manual_seed(13)
    T = 64 * 129 + 1
    check([Layer(gen, T, di, do, r, dtype, variant) for di, do, r in GROUP4], f"group4 {variant}")


@pytest.mark.parametrize("variant", ["plain", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_four_siblings_shared_input(dtype, variant):
    """The same size through sow_forward_shared / sow_backward_shared (chain2_shared.hip: park form, Y store policy and grid
    are chosen by the same switches): four siblings on one x, one dX."""
    gen = torch.Generator(device=DEV).manual_seed(17)
    T = 64 * 129 + 1
    first = Layer(gen, T, 64, 64, 8, dtype, variant)
    sibs = [first] + [Layer(gen, T, 64, do, r, dtype, variant, x=first.x, dxbuf=first.dxbuf) for do, r in ((192, 64), (72, 50), (128, 16))]
    check(sibs, f"shared4 {variant}", shared=True)


BLOCK = [(512, 512)] * 4 + [(512, 1376)] * 2 + [(1376, 512)]
TN_POLICIES = [dict(TN_NO_NT_LOAD=1), dict(NO_H_ROWS=1), dict(NT_LOAD=1), dict(NO_PERSIST=1)]


@pytest.mark.parametrize("T,shapes,rows", [(2048, [(64, 64), (512, 1376)], False), (8192, BLOCK, True)], ids=["T2048-pair", "T8192-block"])
def test_weight_gradients_do_not_depend_on_the_m_stream_policy(T, shapes, rows):
    """dA / dB of a grouped call, bit for bit, with M streamed or cached, and from h_save / dh written either way.  The row-owner kernel takes groups that fill 160 ..
    256 blocks with slabs of at least 512 tokens (tn_rows_plan): the two-layer group at T = 2048 stays on the column-owner
    kernels (which have no policy), so a whole decoder block at T = 8192 is the launch that runs it."""
    gen = torch.Generator(device=DEV).manual_seed(3)
    layers = [Layer(gen, T, di, do, 50, torch.bfloat16, "plain") for di, do in shapes]
    grp = ops.LayerGroup([L.call for L in layers])
    with _lib.switch(NO_TN_ROWS=0, NO_GROUPED=0, TN_NARROW=0):
        assert bool(grp.weight_gradient_plan()[0]) == rows
        run(layers, NEW, _lib.BWD_DATA | _lib.BWD_WEIGHTS)
        want = [(L.dA.clone(), L.dB.clone()) for L in layers]
        for L, (dA, dB) in zip(layers, want):
            x, dy = to64(L.x), to64(L.dy)
            h, dh = to64(L.hbuf[:T * 64].view(T, 64)[:, :50]), to64(L.dh()[:, :50])
            for got, ref in ((dA, x.t() @ dh), (dB, h.t() @ dy)):
                assert float((to64(got) - ref).abs().max() / ref.abs().max()) < 6e-3   # bf16 gradients of the kernels' own h / dh
        for sw in TN_POLICIES:
            for L in layers:
                L.dA.fill_(float("nan")), L.dB.fill_(float("nan"))
            run(layers, dict(NEW, **sw), _lib.BWD_DATA | _lib.BWD_WEIGHTS)
            for li, (L, (dA, dB)) in enumerate(zip(layers, want)):
                assert torch.equal(L.dA, dA) and torch.equal(L.dB, dB), f"layer {li}: weight gradients differ under {sw}"
