"""-m gpu: the paired X issue of the chain kernel (chain2.hip: c2_x_issued, NO_X_PAIR switch).

The compute waves of a token group issue their X stages two at a time, after the barrier of every even stage, so that 256
contiguous bytes of a token row are requested back to back; NO_X_PAIR = 1 issues one stage per barrier as before.  Slot,
LDS image and k order of a stage are the same under both rules, so y, h_save, dX, dh and every workspace byte must be equal
bit for bit between the two -- in NaN-poisoned buffers with guard rows past T and an odd workspace offset (the Layer of
tests/test_gpu_row_align.py).  A wait that counts one stage too many reads a stage still in flight, an issue one barrier early
overwrites a stage the partner wave still reads: both show as different bits, or as NaN left of the poison.  The default is
also held element by element to float64 with the checks the element-wise tests apply to this kernel (tests/numerics.py):
h_save and dh with check_h_save, y and dX as RNE of the product of the VISIBLE h / dh with the fp32 accumulation floor.

Cases, one per place the schedule can go wrong:
  stage counts 1, 2, 3, 4, 5, 8, 9 (square layers: the backward runs the same count on dY): an odd tail, a prologue shorter and
  longer than the ring; a ragged last stage (200 columns; ranks 50 and 8); the row-aligned widths 1376 -> 512 and 512 -> 1376
  (shifted stages in pairs; NO_SHORT_SPLIT keeps them in one launch at this T), bf16 and f16; T = 64, 100 and 4160 (guarded
  rows in the last block); four layers in one grid at T = 16384 (1024 blocks on 512 resident workgroups: the ring is reused
  across blocks); the short-T split at T = 2048, 1376 -> 512 (pairs inside a workgroup's own stage range); one case captured in
  a HIP graph and replayed three times in place."""
import pytest
import torch

from numerics import UNIT_ROUNDOFF, accumulation_term, check_h_save, fp32_floor, to64
from sow_amd import _lib, ops
from test_gpu_row_align import SCALE, Layer, rounded, run

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
NAMES = ("y", "h_save", "dX", "workspace (dh)")


def against_float64(layers, tag):
    u32 = UNIT_ROUNDOFF[torch.float32]
    for L in layers:
        T, dt = L.T, L.dtype
        for name, buf, width in (("y", L.ybuf, L.d_out), ("h_save", L.hbuf, 64), ("dX", L.dxbuf, L.d_in)):
            assert (buf.view(torch.int16)[T * width:] == -1).all(), f"{tag}: {name} written past row T"
            assert not torch.isnan(buf[:T * width]).any(), f"{tag}: {name} has unwritten elements below row T"
        x, dy, A, B = to64(L.x), to64(L.dy), to64(L.A), to64(L.B)
        check_h_save(L.hbuf[:T * 64], SCALE * (x @ A), L.r, dt, acc=accumulation_term(SCALE * SCALE * ((x * x) @ (A * A)), u32, L.d_in),
                     name=f"{tag}: h_save")
        check_h_save(L.dh(), SCALE * (dy @ B.t()), L.r, dt, acc=accumulation_term(SCALE * SCALE * ((dy * dy) @ (B * B).t()), u32, L.d_out),
                     name=f"{tag}: dh")
        h = to64(L.hbuf[:T * 64].view(T, 64)[:, :L.r])
        dh = to64(L.dh()[:, :L.r])
        rounded(L.ybuf[:T * L.d_out].view(T, L.d_out), h @ B, dt, fp32_floor((h * h) @ (B * B), L.d_in + 64), f"{tag}: y")
        rounded(L.dxbuf[:T * L.d_in].view(T, L.d_in), dh @ A.t(), dt, fp32_floor((dh * dh) @ (A * A).t(), L.d_out + 64), f"{tag}: dX")


def same(new, other, tag, what):
    for li, (a, b) in enumerate(zip(new, other)):
        for name, u, v in zip(NAMES, a, b):
            assert torch.equal(u, v), f"{tag}: {name} of layer {li} differs from {what}"


def check(layers, tag, base=None):
    base = base or {}
    new = run(layers, dict(base, NO_X_PAIR=0))
    against_float64(layers, tag)
    same(new, run(layers, dict(base, NO_X_PAIR=1)), tag, "the run with NO_X_PAIR=1")
    return new


STAGES = [64, 128, 192, 256, 320, 512, 576]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("d", STAGES, ids=[f"{d // 64}-stages" for d in STAGES])
def test_stage_counts(d, dtype):
    gen = torch.Generator(device=DEV).manual_seed(7000 + d)
    check([Layer(gen, 130, d, d, 50, dtype, "plain")], f"T=130 {d}->{d}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("r", [50, 8])
def test_ragged_last_stage(r, dtype):
    gen = torch.Generator(device=DEV).manual_seed(7100 + r)
    check([Layer(gen, 130, 200, 200, r, dtype, "plain")], f"T=130 200->200 r={r}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("widths", [(1376, 512), (512, 1376)], ids=["1376x512", "512x1376"])
def test_row_aligned_widths(widths, dtype):
    gen = torch.Generator(device=DEV).manual_seed(7200 + widths[0])
    L = [Layer(gen, 192, *widths, 50, dtype, "plain")]
    new = check(L, f"T=192 {widths}", base=dict(NO_SHORT_SPLIT=1))
    # ... and the unshifted stages of the same widths
    same(new, run(L, dict(NO_SHORT_SPLIT=1, NO_ROW_ALIGN=1)), f"T=192 {widths}", "the run with NO_ROW_ALIGN=1")


@pytest.mark.parametrize("T", [64, 100, 4160])
def test_token_counts(T):
    gen = torch.Generator(device=DEV).manual_seed(7300 + T)
    check([Layer(gen, T, 320, 256, 50, torch.bfloat16, "plain")], f"T={T} 320->256")


def test_two_rounds_of_a_persistent_grid():
    """Four layers at T = 16384 share one grid of 1024 blocks: every resident workgroup runs two, of different stage counts."""
    gen = torch.Generator(device=DEV).manual_seed(7400)
    T = 16384
    check([Layer(gen, T, 192, 128, 50, torch.bfloat16, "plain"), Layer(gen, T, 128, 320, 64, torch.bfloat16, "plain"),
           Layer(gen, T, 320, 64, 50, torch.bfloat16, "plain"), Layer(gen, T, 64, 192, 8, torch.bfloat16, "plain")], "group of four, T=16384")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_short_split(dtype):
    gen = torch.Generator(device=DEV).manual_seed(7500)
    check([Layer(gen, 2048, 1376, 512, 50, dtype, "plain")], "T=2048 1376->512, short-T split")


def test_graph_replay():
    gen = torch.Generator(device=DEV).manual_seed(7600)
    L = [Layer(gen, 130, 320, 576, 50, torch.bfloat16, "plain")]
    eager = check(L, "T=130 320->576 (eager)")
    grp = ops.LayerGroup([l.call for l in L])

    def step():
        grp.forward()
        grp.backward(_lib.BWD_DATA)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for i in range(3):
        L[0].poison()
        graph.replay()
        torch.cuda.synchronize()
        same([L[0].snapshot()], eager, f"replay {i}", "the eager run")
