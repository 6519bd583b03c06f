"""-m gpu: the line-aligned X stages and Y slices of the chain kernel (chain2.hip, NO_ROW_ALIGN switch).

Where a 16-bit row pitch is 64 bytes past a multiple of 128 (width % 64 == 32: 96, 160, 1376), the two token groups of a
workgroup become the even and the odd rows of its block and the odd group cuts its X stages (read side) and its Y slices
(write side) 32 columns early.  None of this touches a value: y, h_save, dX, dh and every workspace byte must equal, bit
for bit, what NO_ROW_ALIGN = 1 (both sides off), = 2 (read side off) and = 3 (write side off) leave, in NaN-poisoned
buffers with guard rows past T -- an unwritten half-slice at a row end, the predicated-off first half-stage and a row that
lands at another token's index all show there.  The same outputs are held element by element to float64 with the checks
the element-wise tests apply to this kernel (tests/numerics.py): h_save and dh with check_h_save, y and dX as RNE of the
product of the VISIBLE h / dh with the fp32 accumulation floor of their sums.

Shapes: widths 96 and 160 (1.5 and 2.5 chunks) against a 128-wide partner on the read side, the write side and on both
(the backward swaps the sides); T = 64 (one block), 130 (ragged tail whose last row is odd) and 192; ranks 50 and 64; bf16
and f16; the fp32-park epilogue (bias; beta = 1 after a low-rank accumulator), where only the read side and the row
parity apply; 512 -> 1376 and 1376 -> 512 at T = 128 with and without the short-T split (the split keeps the unshifted
code); a two-layer launch of which one layer qualifies (T > 8192: below it layers do not share a launch); more blocks than
resident workgroups (a workgroup runs two blocks: the ring slots are reused across blocks).  The C ABI takes contiguous
rows, so a pitch larger than the width cannot be reached from here; 128-wide layers are the pitch that does not qualify."""
import pytest
import torch

from numerics import MAX_INEXACT, UNIT_ROUNDOFF, accumulation_term, check_h_save, check_rounded, fp32_floor, rne, to64, ulp
from sow_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
TAIL = 64        # guard rows past T in every output buffer
SCALE = 0.75
OFF = [("both sides off", dict(NO_ROW_ALIGN=1)), ("read side off", dict(NO_ROW_ALIGN=2)), ("write side off", dict(NO_ROW_ALIGN=3))]


class Layer:
    """One layer's operands, NaN-filled outputs with TAIL guard rows, and a 0xFF-filled workspace."""

    def __init__(self, gen, T, d_in, d_out, r, dtype, variant):
        def rnd(*shape, s=1.0):
            return (torch.randn(*shape, generator=gen, device=DEV) * s).to(dtype)
        self.T, self.d_in, self.d_out, self.r, self.dtype, self.variant = T, d_in, d_out, r, dtype, variant
        self.x, self.dy = rnd(T, d_in), rnd(T, d_out)
        self.A, self.B = rnd(d_in, r, s=0.05), rnd(r, d_out, s=0.05)
        self.bias = rnd(d_out) if variant == "bias" else None
        self.acc = (rnd(d_in, 8, s=0.05), rnd(8, d_out, s=0.05)) if variant == "beta" else (None, None)
        self.ybuf = torch.empty((T + TAIL) * d_out, dtype=dtype, device=DEV)
        self.hbuf = torch.empty((T + TAIL) * 64, dtype=dtype, device=DEV)
        self.dxbuf = torch.empty((T + TAIL) * d_in, dtype=dtype, device=DEV)
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


def run(layers, switches):
    grp = ops.LayerGroup([L.call for L in layers])
    for L in layers:
        L.poison()
    with _lib.switch(**switches):
        grp.forward()
        grp.backward(_lib.BWD_DATA)
    torch.cuda.synchronize()
    return [L.snapshot() for L in layers]


def rounded(out, ref, dt, acc, name):
    """check_rounded with the f16 allowance of the element-wise tests: the share of elements allowed off RNE(ref64) grows by
    the mean of acc / ulp (an f16 ulp is 8x finer than a bf16 one)."""
    if dt != torch.float16:
        return check_rounded(out, ref, dt, acc=acc, name=name)
    share = float((to64(acc) / ulp(rne(to64(ref), dt), dt)).clamp(max=1.0).mean())
    return check_rounded(out, ref, dt, acc=acc, max_inexact=MAX_INEXACT + share, name=name)


def check(layers, tag, base=None):
    base = base or {}
    new = run(layers, dict(base, NO_ROW_ALIGN=0))
    # rows past T keep the NaN pattern; every element below row T was written
    for L in layers:
        T = L.T
        for name, buf, width in (("y", L.ybuf, L.d_out), ("h_save", L.hbuf, 64), ("dX", L.dxbuf, L.d_in)):
            assert (buf.view(torch.int16)[T * width:] == -1).all(), f"{tag}: {name} written past row T"
            assert not torch.isnan(buf[:T * width]).any(), f"{tag}: {name} has unwritten elements below row T"
    u32 = UNIT_ROUNDOFF[torch.float32]
    for L in layers:
        T, dt = L.T, L.dtype
        x, dy, A, B = to64(L.x), to64(L.dy), to64(L.A), to64(L.B)
        # h_save = RNE(s x A), dh = RNE(s dY B^T); zeros in r..62, 1.0 in column 63 when it is free
        check_h_save(L.hbuf[:T * 64], SCALE * (x @ A), L.r, dt, acc=accumulation_term(SCALE * SCALE * ((x * x) @ (A * A)), u32, L.d_in),
                     name=f"{tag}: h_save")
        check_h_save(L.dh(), SCALE * (dy @ B.t()), L.r, dt, acc=accumulation_term(SCALE * SCALE * ((dy * dy) @ (B * B).t()), u32, L.d_out),
                     name=f"{tag}: dh")
        # y = RNE(h B + bias) and dX = RNE(dh A^T) from the visible h / dh (the low-rank accumulator's first term is rounded
        # before the chain adds to it: that variant is held bit for bit only)
        h = to64(L.hbuf[:T * 64].view(T, 64)[:, :L.r])
        dh = to64(L.dh()[:, :L.r])
        if L.variant != "beta":
            y_ref = h @ B + (to64(L.bias) if L.bias is not None else 0)
            rounded(L.ybuf[:T * L.d_out].view(T, L.d_out), y_ref, dt, fp32_floor((h * h) @ (B * B), L.d_in + 64), f"{tag}: y")
            rounded(L.dxbuf[:T * L.d_in].view(T, L.d_in), dh @ A.t(), dt, fp32_floor((dh * dh) @ (A * A).t(), L.d_out + 64), f"{tag}: dX")
    for name, sw in OFF:
        other = run(layers, dict(base, **sw))
        for li, (a, b) in enumerate(zip(new, other)):
            for what, u, v in zip(("y", "h_save", "dX", "workspace (dh)"), a, b):
                assert torch.equal(u, v), f"{tag}: {what} of layer {li} differs from the run with {name}"


WIDTHS = [(96, 128), (160, 128), (128, 96), (128, 160), (96, 160), (160, 96)]
CASES = [(T, w, r) for T in (64, 130, 192) for w in WIDTHS for r in (50, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("T,widths,r", CASES, ids=[f"T{t}-{w[0]}x{w[1]}r{r}" for t, w, r in CASES])
def test_single_layer(T, widths, r, dtype):
    gen = torch.Generator(device=DEV).manual_seed(2000 + T + widths[0] + r)
    check([Layer(gen, T, *widths, r, dtype, "plain")], f"T={T} {widths} r={r}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("variant", ["bias", "beta"])
@pytest.mark.parametrize("widths", [(96, 160), (160, 96)], ids=["96x160", "160x96"])
def test_fp32_park_epilogue(widths, variant, dtype):
    """bias / beta = 1 take chain2_kernel<., false>: row parity and the read side apply, the slices stay unshifted."""
    gen = torch.Generator(device=DEV).manual_seed(31 + widths[0])
    check([Layer(gen, 130, *widths, 50, dtype, variant)], f"T=130 {widths} {variant}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("split", [True, False], ids=["short-split", "one-launch"])
@pytest.mark.parametrize("widths", [(512, 1376), (1376, 512)], ids=["512x1376", "1376x512"])
def test_headline_widths(widths, split, dtype):
    gen = torch.Generator(device=DEV).manual_seed(41 + widths[0])
    check([Layer(gen, 128, *widths, 50, dtype, "plain")], f"T=128 {widths} split={split}", base={} if split else dict(NO_SHORT_SPLIT=1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_group_of_which_one_layer_qualifies(dtype):
    """T > 8192: the two layers share one grid (130 blocks each); the 128-wide one runs the aligned kernel's unshifted arithmetic."""
    gen = torch.Generator(device=DEV).manual_seed(53)
    T = 64 * 129 + 9
    check([Layer(gen, T, 96, 160, 50, dtype, "plain"), Layer(gen, T, 128, 128, 64, dtype, "plain")], "group 96x160 + 128x128")


def test_more_blocks_than_resident_workgroups():
    gen = torch.Generator(device=DEV).manual_seed(59)
    check([Layer(gen, 64 * 513 + 9, 160, 96, 50, torch.bfloat16, "plain")], "T=64*513+9 160->96")
