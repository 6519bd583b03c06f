"""-m gpu: which kernel computes the weight gradients of a layer, one row per TnKernel (kernels.hpp) at the smallest shape that
reaches it, under the defaults and under the switches of the selection rule (skinny_tn.hip: tn_shape_kernel / pick_tn; api.hip:
pick_tn_wide_rank and the grouped arms of backward_group_impl).  Each row asserts the kernel's name (torch.profiler, as
test_gpu_gemm_selection.py) and dA, dB and dbias element by element against the float64 products with check_rounded.

The calls run the weight phases alone (SOW_BWD_WEIGHTS): the test itself puts dh where the data phase leaves it (the head of
the aligned workspace) and h_save in the chain kernels' contract (zeros from column r on, 1.0 in column 63 for r <= 63), so
both operands of both products are tensors the test holds and the references are exact:
    dA = x^T dh,  dB = h^T dY,  dbias = colsum(dY),  each an fp32 sum over T rounded once.
bf16 / f16: check_rounded as it stands (one ulp of RNE(ref64) plus the fp32 floor of a T-term sum, at most 0.5 % of the
elements off RNE).  fp32: the same limit, with every element allowed off RNE (max_inexact = 1: an fp32 sum of fp32 products is
not correctly rounded anywhere) -- the bound of the fp32 cases of test_gpu_elementwise.py.

The table was recorded from the library as it stood before the selector was introduced (SOW_AMD_LIB); the same table holds
after.  ROWS_T is the smallest T at which that library's sow_backward_group_plan put the seven-layer block on the row-owner
kernel (found on the CPU; test_rows_threshold holds it)."""
import ctypes
import functools

import pytest
import torch

import test_gpu_elementwise as E
from numerics import check_rounded, fp32_floor
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {F32: _lib.F32, BF16: _lib.BF16, F16: _lib.F16}
FAMILY = ("tn_partial_kernel", "tn_partial_dma_kernel", "tn_partial_dma_wide_kernel", "tn_partial_rows_kernel",
          "tn_partial_dma_f32_kernel", "tn_partial_dma_f32_wide_kernel", "tn_partial_f32_quad_kernel", "tnw_partial_kernel",
          "gemm_kernel")
SWITCHES = ("TN_NARROW", "F32_EXACT", "NO_TN_F32Q", "NO_F16_TN", "NO_TN_ROWS", "NO_GROUPED", "NO_WIDE_CHAIN", "NO_RAGGED")
BLOCK = [(512, 512)] * 4 + [(512, 1376)] * 2 + [(1376, 512)]
ROWS_T = 5120

# (id, dtype, T, (d_in, d_out), r, x offset in elements, switches, kernel, template argument or None)
CASES = [
    ("bf16_default", BF16, 1024, (512, 512), 50, 0, {}, "tn_partial_dma_wide_kernel", None),
    ("bf16_narrow", BF16, 1024, (512, 512), 50, 0, dict(TN_NARROW=1), "tn_partial_dma_kernel", None),
    ("bf16_x_offset", BF16, 1024, (512, 512), 50, 1, {}, "tn_partial_kernel", None),
    ("f16_default", F16, 1024, (512, 512), 50, 0, {}, "tn_partial_dma_wide_kernel", None),
    ("f16_narrow", F16, 1024, (512, 512), 50, 0, dict(TN_NARROW=1), "tn_partial_dma_kernel", None),
    ("f16_x_offset", F16, 1024, (512, 512), 50, 1, {}, "tn_partial_kernel", None),
    ("f16_no_f16_tn", F16, 1024, (512, 512), 50, 0, dict(NO_F16_TN=1), "tn_partial_kernel", None),
    ("f32_quad", F32, 4096, (192, 192), 50, 0, {}, "tn_partial_f32_quad_kernel", None),
    ("f32_no_quad", F32, 4096, (192, 192), 50, 0, dict(NO_TN_F32Q=1), "tn_partial_dma_f32_wide_kernel", None),
    ("f32_exact", F32, 4096, (192, 192), 50, 0, dict(F32_EXACT=1), "tn_partial_dma_f32_kernel", False),
    ("f32_narrow", F32, 4096, (192, 192), 50, 0, dict(TN_NARROW=1), "tn_partial_dma_f32_kernel", True),
    ("f32_T1024", F32, 1024, (192, 192), 50, 0, {}, "tn_partial_dma_f32_wide_kernel", None),
    ("f32_102x36", F32, 1024, (102, 36), 50, 0, {}, "tn_partial_kernel", None),
    ("wide_r66", BF16, 1024, (512, 512), 66, 0, {}, "tnw_partial_kernel", None),
    ("wide_r66_no_wide_chain", BF16, 1024, (512, 512), 66, 0, dict(NO_WIDE_CHAIN=1), "gemm_kernel", None),
    ("wide_r200", BF16, 1024, (512, 512), 200, 0, {}, "tnw_partial_kernel", None),
    ("wide_r200_no_wide_chain", BF16, 1024, (512, 512), 200, 0, dict(NO_WIDE_CHAIN=1), "gemm_kernel", None),
    ("ragged_100x36", BF16, 1024, (100, 36), 66, 0, {}, "tnw_partial_kernel", None),
    ("ragged_100x36_no_ragged", BF16, 1024, (100, 36), 66, 0, dict(NO_RAGGED=1), "gemm_kernel", None),
]


def _h_contract(t, r):
    """[T, max(r, 64)] in the chain kernels' contract for r <= 64: zeros from column r on, 1.0 in column 63 when r <= 63."""
    if r <= 64:
        t[:, r:] = 0
        if r <= 63:
            t[:, 63] = 1
    return t


@functools.lru_cache(maxsize=8)   # the rows of one shape and dtype are neighbours; the block has five operand sets
def _operands(dtype, T, d_in, d_out, r, seed=0):
    """x (with one spare element in front), dY, h_save, dh in `dtype` on the GPU and the three float64 references with their
    fp32 floors, on the CPU.  Shared by the rows of a shape; nobody writes to them."""
    g = torch.Generator().manual_seed(T + d_in + d_out + r + seed)
    hc = max(r, 64)
    xbuf = torch.randn(T * d_in + 8, generator=g).to(dtype).to(DEV)
    dy = torch.randn(T, d_out, generator=g).to(dtype).to(DEV)
    h = _h_contract(torch.randn(T, hc, generator=g) * 0.5, r).to(dtype).to(DEV)
    dh = _h_contract(torch.randn(T, hc, generator=g) * 0.5, r).to(dtype).to(DEV)
    refs = {}
    for off in (0, 1):
        x64 = xbuf[off:off + T * d_in].view(T, d_in).double()
        refs[off] = ((x64.t() @ dh.double()[:, :r]).cpu(), fp32_floor(((x64 * x64).t() @ (dh.double()[:, :r] ** 2)).cpu(), T))
    h64, dy64 = h.double()[:, :r], dy.double()
    refs["dB"] = ((h64.t() @ dy64).cpu(), fp32_floor(((h64 * h64).t() @ (dy64 * dy64)).cpu(), T))
    refs["dbias"] = (dy64.sum(0).cpu(), fp32_floor((dy64 * dy64).sum(0).cpu(), T))
    return xbuf, dy, h, dh, refs


def _workspace(dtype, T, d_in, d_out, r, dh):
    """A poisoned workspace (sized under the switches in force) with dh at the head of its 256-byte-aligned part."""
    n = _lib.load().sow_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, DT[dtype])
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)
    start = (-ws.data_ptr()) % 256
    ws[start:start + dh.numel() * dh.element_size()] = dh.reshape(-1).view(torch.uint8)
    return ws


def _ran(seq):
    return [k for k in FAMILY if E._has_kernel(seq, k)]


def _template_arg(seq, kernel):
    """True / False: the bool template argument of the one instantiation of `kernel` in the trace (mangled or demangled)."""
    names = {n for n in seq if E._has_kernel([n], kernel)}
    assert len(names) == 1, names
    n = names.pop()
    return "Lb1" in n or "<true>" in n or "(bool)1" in n


def _check(name, dtype, out, ref, acc):
    st = check_rounded(out.cpu(), ref, dtype, acc=acc, name=name, **(dict(max_inexact=1.0) if dtype == F32 else {}))
    print(f"{name}: worst err/limit {st['worst']:.3f}, inexact {100 * st['inexact']:.4f} %")


@pytest.mark.parametrize("name,dtype,T,widths,r,xoff,switches,kernel,targ", CASES, ids=[c[0] for c in CASES])
def test_tn_selection(name, dtype, T, widths, r, xoff, switches, kernel, targ):
    lib = _lib.load()
    d_in, d_out = widths
    xbuf, dy, h, dh, refs = _operands(dtype, T, d_in, d_out, r)
    x = xbuf[xoff:xoff + T * d_in].view(T, d_in)
    nan = float("nan")
    dA = torch.full((d_in, r), nan, dtype=dtype, device=DEV)
    dB = torch.full((r, d_out), nan, dtype=dtype, device=DEV)
    dbias = torch.full((d_out,), nan, dtype=dtype, device=DEV)
    dx = torch.empty(8, dtype=dtype, device=DEV)    # not written: no data phase
    with _lib.switch(**switches):
        ws = _workspace(dtype, T, d_in, d_out, r, dh)

        def call():
            _lib.check(lib.sow_backward_ex(dy.data_ptr(), x.data_ptr(), h.data_ptr(), dx.data_ptr(), dx.data_ptr(), None, None,
                                           dx.data_ptr(), dA.data_ptr(), dB.data_ptr(), dbias.data_ptr(), T, d_in, d_out, r, 0,
                                           _lib.ACC_NONE, 1.0, 0.0, DT[dtype], ws.data_ptr(), ws.numel(), _lib.BWD_WEIGHTS,
                                           E._stream()), "sow_backward_ex")

        seq = E._kernel_seq(call)
    assert all(lib.sow_get_switch(k.encode()) == -1 for k in SWITCHES)
    ran = _ran(seq)
    print(f"{name}: {ran} {sorted(set(seq))}")
    assert ran == [kernel], f"{name}: expected {kernel} alone, the trace shows {ran}: {sorted(set(seq))}"
    if targ is not None:
        assert _template_arg(seq, kernel) == targ, f"{name}: {sorted(set(seq))}"
    _check(f"{name}: dA", dtype, dA, *refs[xoff])
    _check(f"{name}: dB", dtype, dB, *refs["dB"])
    _check(f"{name}: dbias", dtype, dbias, *refs["dbias"])


# ---- the seven-layer block through sow_backward_group (weight phases alone: bf16 plans the row-owner kernel for them)
# (id, switches, kernel, launches of it)
GROUPED = [
    ("block_rows", {}, "tn_partial_rows_kernel", 1),
    ("block_no_tn_rows", dict(NO_TN_ROWS=1), "tn_partial_dma_wide_kernel", 1),
    ("block_no_grouped", dict(NO_GROUPED=1), "tn_partial_dma_wide_kernel", 7),
]


def _block_args(lib, T, bufs=None):
    """LayerArgs of the block at T rows: fake 16-byte-aligned pointers (plan queries), or the tensors of `bufs`."""
    arr = (_lib.LayerArgs * len(BLOCK))()
    for i, (d_in, d_out) in enumerate(BLOCK):
        b = bufs[i] if bufs else {}
        p = {k: (b[k].data_ptr() if bufs else 1 << 20) for k in ("x", "dy", "h", "dA", "dB", "dbias", "ws", "dx")}
        n = b["ws"].numel() if bufs else lib.sow_workspace_bytes(T, d_in, d_out, 50, 0, _lib.ACC_NONE, _lib.BF16) + 256
        arr[i] = _lib.LayerArgs(x=p["x"], A=p["dx"], B=p["dx"], y=p["dx"], h_save=p["h"], dy=p["dy"], dx=p["dx"], dA=p["dA"],
                                dB=p["dB"], dbias=p["dbias"], T=T, d_in=d_in, d_out=d_out, r_live=50, r_acc=0,
                                acc_kind=_lib.ACC_NONE, scale=1.0, grad_beta=0.0, workspace=p["ws"], workspace_bytes=n)
    return arr


def _rows_planned(lib, T):
    slabs = (ctypes.c_int * (2 * len(BLOCK)))()
    return lib.sow_backward_group_plan(_block_args(lib, T), len(BLOCK), _lib.BF16, _lib.BWD_WEIGHTS, slabs)


def test_rows_threshold():
    lib = _lib.load()
    assert _rows_planned(lib, ROWS_T) == 1
    assert not any(_rows_planned(lib, T) for T in range(1, ROWS_T))


@pytest.mark.parametrize("name,switches,kernel,launches", GROUPED, ids=[g[0] for g in GROUPED])
def test_tn_group_selection(name, switches, kernel, launches):
    lib = _lib.load()
    T, nan = ROWS_T, float("nan")
    bufs = []
    with _lib.switch(**switches):
        for i, (d_in, d_out) in enumerate(BLOCK):
            xbuf, dy, h, dh, refs = _operands(BF16, T, d_in, d_out, 50, seed=i % 4 if d_in == d_out else 0)
            bufs.append(dict(x=xbuf[:T * d_in].view(T, d_in), dy=dy, h=h, refs=refs, ws=_workspace(BF16, T, d_in, d_out, 50, dh),
                             dA=torch.full((d_in, 50), nan, dtype=BF16, device=DEV),
                             dB=torch.full((50, d_out), nan, dtype=BF16, device=DEV),
                             dbias=torch.full((d_out,), nan, dtype=BF16, device=DEV), dx=torch.empty(8, dtype=BF16, device=DEV)))
        arr = _block_args(lib, T, bufs)
        seq = E._kernel_seq(lambda: _lib.check(lib.sow_backward_group(arr, len(BLOCK), _lib.BF16, _lib.BWD_WEIGHTS, E._stream()),
                                               "sow_backward_group"))
    assert all(lib.sow_get_switch(k.encode()) == -1 for k in SWITCHES)
    ran = _ran(seq)
    print(f"{name}: {ran} {sorted(set(seq))}")
    assert ran == [kernel], f"{name}: expected {kernel} alone, the trace shows {ran}: {sorted(set(seq))}"
    assert sum(E._has_kernel([n], kernel) for n in seq) == launches, f"{name}: {seq}"
    for i, b in enumerate(bufs):
        _check(f"{name}[{i}]: dA", BF16, b["dA"], *b["refs"][0])
        _check(f"{name}[{i}]: dB", BF16, b["dB"], *b["refs"]["dB"])
        _check(f"{name}[{i}]: dbias", BF16, b["dbias"], *b["refs"]["dbias"])
