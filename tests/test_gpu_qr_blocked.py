"""-m gpu: the blocked Householder QR of sow_qr_thin (sow_amd/csrc/qr_blocked.hip: more than 64 factored columns).

1. numerics: check_qr (tests/step_numerics.py, the committed bounds) against float64 / LAPACK through the guarded, poisoned
   Arena of test_gpu_step_elementwise.py (three runs, bit-identical) for square, tall, wide, complete-mode, partial-block,
   scaled, Q-only and pitched cases (QR_BLOCKED_CASES of test_qr_blocked_cpu.py, where the fp32 emulation passes them too);
2. rank-deficient inputs, among them zero columns on both sides of a block boundary: no NaN, bounds met;
3. the route (torch profiler): qr_larfb_kernel past 64 columns, not under NO_BLOCKED_QR = 1, not at k = 50, whose outputs
   do not depend on the switch;
4. the Python surface: SoWLinear.accumulate() on the low-rank branch and prepare_sow(decompose='qr');
5. a sanity condition on speed: the blocked route is faster than the one-workgroup route at 1001 x 1001.
"""
import statistics

import pytest
import torch
from torch import nn

from conftest import rel_err
from step_numerics import check_qr
from test_gpu_step_elementwise import _note, _run_qr
from test_qr_blocked_cpu import QR_BLOCKED_CASES, RANK_DEFICIENT, case_input, rank_deficient_input
from sow_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
QR_TOL = 5e-5   # tests/test_gpu_parity.py: Householder outputs of two summation orders


@pytest.mark.parametrize("m,n,k,din,dout,need_r,extra_ld,scale", QR_BLOCKED_CASES)
def test_blocked_qr_against_fp64(m, n, k, din, dout, need_r, extra_ld, scale):
    W0 = case_input(m, n, k, din, scale)
    name = f"blocked qr {m}x{n} k={k}"
    out, dt = _run_qr(W0, k, dout, need_r, extra_ld, name)
    st = check_qr(W0, out["Q"], out.get("R"), k, dout, name=name)
    _note(f"{name} {din}->{dout} need_r={need_r} ld+{extra_ld} scale={scale:g} ({1e3 * dt:.0f} ms/call)", st)


@pytest.mark.parametrize("kind", RANK_DEFICIENT)
def test_blocked_qr_rank_deficient(kind):
    W0 = rank_deficient_input(kind)
    out, _ = _run_qr(W0, 80, F32, 1, 0, f"blocked qr {kind}")
    _note(f"blocked qr {kind}", check_qr(W0, out["Q"], out["R"], 80, F32, name=f"blocked qr {kind}", against_lapack=False))


# ---- route ----------------------------------------------------------------------------------------------------------------
def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


def _has(names, kernel):
    return any(f"sow::{kernel}" in n or f"{len(kernel)}{kernel}" in n for n in names)


def test_wide_panels_run_the_blocked_kernels():
    W = torch.randn(200, 200, generator=torch.Generator().manual_seed(5)).to(DEV)
    ops.qr_thin(W, 200)   # warm-up: library loaded, workspace allocated
    names = _kernel_names(lambda: ops.qr_thin(W, 200))
    assert names, "the profiler recorded no GPU kernels"
    assert _has(names, "qr_larfb_kernel") and _has(names, "qr_block_panel_kernel"), sorted(names)
    assert not _has(names, "qr_panel_kernel"), sorted(names)
    with _lib.switch(NO_BLOCKED_QR=1):
        names = _kernel_names(lambda: ops.qr_thin(W, 200))
    assert _has(names, "qr_panel_kernel") and not _has(names, "qr_larfb_kernel"), sorted(names)
    # 50 columns: the one-workgroup panel whatever the switch says, the same bits
    names = _kernel_names(lambda: ops.qr_thin(W, 50))
    assert _has(names, "qr_panel_kernel") and not _has(names, "qr_larfb_kernel"), sorted(names)
    q0, r0 = ops.qr_thin(W, 50)
    with _lib.switch(NO_BLOCKED_QR=1):
        q1, r1 = ops.qr_thin(W, 50)
    assert torch.equal(q0.view(torch.int32), q1.view(torch.int32)) and torch.equal(r0.view(torch.int32), r1.view(torch.int32))
    # 64 factored columns of a wider request (complete mode, kc = n = 64): still the one-workgroup panel
    W64 = W[:, :64].contiguous()
    names = _kernel_names(lambda: ops.qr_thin(W64, 100))
    assert _has(names, "qr_panel_kernel") and not _has(names, "qr_larfb_kernel"), sorted(names)


# ---- surface --------------------------------------------------------------------------------------------------------------
def _accumulate_twice(monkeypatch, switch):
    from sow_amd import SoWLinear
    gen = torch.Generator().manual_seed(21)
    draws = iter([torch.randn(384, 320, generator=gen) * 0.02 for _ in range(3)])
    ups = [torch.randn(96, 320, generator=gen) * 0.05 for _ in range(3)]
    x = torch.randn(64, 384, generator=gen).to(DEV)
    monkeypatch.setattr(SoWLinear, "_fresh_gaussian", lambda self, shape, device, dtype: next(draws).to(device, dtype))
    ranks, ys = [], []
    with _lib.switch(NO_BLOCKED_QR=switch):
        layer = SoWLinear(384, 320, bias=False, rank=96, scale=0.5, init_method="normal_QR", device=DEV)
        assert layer.virtual_rank == 96
        for step in range(3):
            layer.upscale_weights[0].data.copy_(ups[step])   # B moved by training; accumulate() zeroes it again
            with torch.no_grad():
                ys.append(layer(x).cpu())
            if step < 2:
                layer.accumulate()
                assert layer.acc_upweight.numel() != 0, "the accumulator left the low-rank branch"
            ranks.append(layer.virtual_rank)
    return ranks, ys


def test_accumulate_on_the_low_rank_branch(monkeypatch):
    ranks, ys = _accumulate_twice(monkeypatch, 0)
    ranks_ref, ys_ref = _accumulate_twice(monkeypatch, 1)
    assert ranks == ranks_ref == [192, 288, 288]
    for step, (y, y_ref) in enumerate(zip(ys, ys_ref)):
        e = rel_err(y, y_ref)
        print(f"forward after {step} accumulate() calls: rel_err {e:.3g}")
        assert e < QR_TOL, (step, e)


def test_prepare_sow_qr_reproduces_the_weights():
    from sow_amd import SoWConfig, prepare_sow
    torch.manual_seed(4)
    model = nn.Sequential()
    model.add_module("up_proj", nn.Linear(160, 160, bias=False))
    model.add_module("down_proj", nn.Linear(160, 160, bias=True))
    weights = {n: m.weight.data.clone() for n, m in model.named_children()}
    cfg = SoWConfig(target_modules=["up_proj", "down_proj"], rank=16, scale=1.0, init_method="normal_QR", decompose="qr",
                    device=DEV)
    names = _kernel_names(lambda: prepare_sow(model, cfg))
    assert _has(names, "qr_larfb_kernel"), sorted(names)
    for n, layer in model.named_children():
        A, B = layer.downscale_weights[0].data, layer.upscale_weights[0].data
        assert layer.acc_downweight.shape == (160, 160) and A.shape == (160, 16) and B.shape == (16, 160)
        wt = layer.acc_downweight.data.double() + A.double() @ B.double()     # Q[:, :-r] R[:-r] + Q[:, -r:] R[-r:] = W^T
        e = rel_err(wt.cpu(), weights[n].t().double())
        print(f"prepare_sow(decompose='qr') {n}: rel_err {e:.3g}")
        assert e < QR_TOL, (n, e)


# ---- speed ----------------------------------------------------------------------------------------------------------------
def _median_ms(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def test_blocked_route_is_faster_than_one_workgroup():
    """A sanity condition, not a target: at 1001 x 1001 the whole chip has to beat one workgroup (NO_BLOCKED_QR = 1, the
    kernel this library had before)."""
    W = torch.randn(1001, 1001, generator=torch.Generator().manual_seed(6)).to(DEV)
    t_new = _median_ms(lambda: ops.qr_thin(W, 1001))
    with _lib.switch(NO_BLOCKED_QR=1):
        t_old = _median_ms(lambda: ops.qr_thin(W, 1001))
    print(f"qr 1001 x 1001, k = 1001: blocked {t_new:.2f} ms, one workgroup {t_old:.2f} ms ({t_old / t_new:.1f} x)")
    assert t_new < t_old, (t_new, t_old)
