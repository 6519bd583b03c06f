"""-m gpu: the fused low-rank-accumulator pass past 256 columns (SOW_FUSE_ACC_DEEP, chain_deep_acc.hip) through the C ABI,
element by element against float64 (tests/deep_acc_numerics.py, the bound of tests/fused_acc_numerics.py), on NaN-poisoned
memory -- and the permission semantics of the flag: every flagged call outside the admitted set gives the bits of the
unflagged call.

The runner is test_gpu_fused_acc's (guarded views, poisoned / zeroed / poisoned workspaces, three bit-identical runs) with
flags = SOW_FUSE_ACC_DEEP.
"""
import dataclasses

import pytest
import torch

import deep_acc_numerics as DA
import fused_acc_numerics as FA
import fuzz_plan as FP
import test_gpu_elementwise as E
import value_plan as V
from numerics import check_h_save, check_rounded, fp32_floor, rne, to64
from sow_amd import _lib
from test_gpu_fused_acc import TWO_PASS, _data, _run, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
FUSE, DEEP = _lib.FUSE_ACC, _lib.FUSE_ACC_DEEP
WORST = {}
KERNEL = "chain_deep_acc_kernel"


def _deep_trace(trace, name):
    """One pack launch and one deep launch per direction, nothing else that writes y / dX."""
    for ph in ("fwd", "bwd"):
        seq = trace[ph]
        assert sum(KERNEL in k for k in seq) == 1, f"{name} {ph}: not exactly one deep launch in {seq}"
        assert sum("wide_acc_pack_kernel" in k for k in seq) == 1, f"{name} {ph}: not exactly one pack launch in {seq}"
        bad = [k for k in seq if any(t in k for t in TWO_PASS) and KERNEL not in k]
        assert not bad, f"{name} {ph}: unflagged data-path kernels next to the deep one: {bad}"
        assert "wide_acc_pack_kernel" in seq[0] and KERNEL in seq[1], f"{name} {ph}: {seq}"


def _no_deep(trace, name):
    for ph in ("fwd", "bwd"):
        assert not any(KERNEL in k or "wide_acc_pack" in k for k in trace[ph]), f"{name} {ph}: a deep launch in {trace[ph]}"


# ---- element-wise against float64, trace, determinism, no poison left
@pytest.mark.parametrize("c", DA.CASES, ids=lambda c: c.name)
def test_deep_layer_elementwise(c):
    d = _data(c)
    trace = {}
    out = _run(c, d, flags=DEEP, trace=trace)
    _deep_trace(trace, c.name)
    worst = DA.check(c, d, out)
    for k, v in worst.items():
        print(f"worst err/limit {c.name:18s} {k:7s} {v:.3f}")
    WORST.update({(c.name, k): v for k, v in worst.items()})
    # dh, which the weight kernels read: the r <= 64 contract, every byte written
    dy, B = to64(d["dy"]), to64(d["B"])
    ref = c.s * (dy @ B.t())
    st = check_h_save(to64(out["dh"]), ref, c.r, c.dtype, acc=fp32_floor(c.s * c.s * ((dy * dy) @ (B * B).t()), c.d_out),
                      name=f"{c.name}: dh")
    WORST[(c.name, "dh")] = st["worst"]
    for k in ("y", "h", "dx", "dA", "dB", "dbias"):
        assert out[k] is None or not torch.isnan(out[k].float()).any(), f"{c.name}: poison left in {k}"


# chain_wide + chain2 (r_acc = 200), the generic GEMM pair + chain2 (r_acc = 448, and 450: not a multiple of 8)
UNFLAGGED = [DA.BY_NAME["tot258"], DA.BY_NAME["tot512"], DA.BY_NAME["llama60m_racc450"]]


@pytest.mark.parametrize("c", UNFLAGGED, ids=lambda c: c.name)
def test_unflagged_call_runs_the_unflagged_kernels(c):
    """The same call without the flag: no deep launch, and outputs inside the two-pass bound of test_gpu_elementwise."""
    d = _data(c)
    trace = {}
    out = _run(c, d, flags=0, trace=trace)
    _no_deep(trace, c.name)
    for ph in ("fwd", "bwd"):
        assert sum(any(t in k for t in TWO_PASS) for k in trace[ph]) >= 2, f"{c.name} {ph}: {trace[ph]}"
    E._check(dataclasses.replace(c, y_rounds="twice"), d, {k: v for k, v in out.items() if k != "dh"})


@pytest.mark.parametrize("c", [DA.BY_NAME["tot258"], DA.BY_NAME["tot320_r64"]], ids=lambda c: c.name)
def test_h_save_null_gives_the_same_y(c):
    d = _data(c)
    with_h = _run(c, d, flags=DEEP, backward=False)
    trace = {}
    without = _run(c, d, flags=DEEP, save_h=False, trace=trace)
    assert any(KERNEL in k for k in trace["fwd"])
    _same_bits(with_h, without, c.name + ": h_save = NULL", keys=("y",))
    DA.check(c, d, dict(y=without["y"]))


# ---- grouped entry points
@pytest.mark.parametrize("c", [DA.BY_NAME["straddle_256"], DA.BY_NAME["tot300_f16"]], ids=lambda c: c.name)
def test_group_fall_through_gives_the_bits_of_the_single_call(c):
    d = _data(c)
    single = _run(c, d, flags=DEEP)
    trace = {}
    grouped = _run(c, d, flags=DEEP, group=True, trace=trace)
    _deep_trace(trace, c.name + " (group)")
    _same_bits(single, grouped, c.name + ": group vs single")


def _group_layer(ar, lib, c, ws_flags):
    d = _data(c)
    b = {k: ar.input(d.get(k)) for k in ("x", "A", "B", "bias", "dy", "Q", "R")}
    b.update(y=ar.output((c.T, c.d_out)), h=ar.output((c.T, 64)), dx=ar.output((c.T, c.d_in)), dA=ar.output((c.d_in, c.r)),
             dB=ar.output((c.r, c.d_out)), dbias=ar.output((c.d_out,)) if c.bias else None)
    b["ws"] = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, _lib.ACC_LOWRANK, _lib.BF16 | ws_flags))
    b["args"] = _lib.LayerArgs(x=E._ptr(b["x"]), A=E._ptr(b["A"]), B=E._ptr(b["B"]), acc_down=E._ptr(b["Q"]), acc_up=E._ptr(b["R"]),
                               bias=E._ptr(b["bias"]), y=E._ptr(b["y"]), h_save=E._ptr(b["h"]), dy=E._ptr(b["dy"]),
                               dx=E._ptr(b["dx"]), dA=E._ptr(b["dA"]), dB=E._ptr(b["dB"]), dbias=E._ptr(b["dbias"]), T=c.T,
                               d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=c.r_acc, acc_kind=_lib.ACC_LOWRANK, scale=c.s,
                               grad_beta=0.0, workspace=E._ptr(b["ws"]), workspace_bytes=b["ws"].numel())
    return b


def _got(b):
    return {k: (None if b[k] is None else b[k].cpu()) for k in ("y", "h", "dx", "dA", "dB", "dbias")}


def test_group_of_two_deep_layers():
    """sow_forward_group / sow_backward_group of two flagged layers: each layer gets the bits of its single call."""
    lib = _lib.load()
    layers = [DA.BY_NAME["tot258"], DA.BY_NAME["straddle_256"]]
    singles = [_run(c, _data(c), flags=DEEP) for c in layers]
    ar = E.Arena(BF16)
    bufs = [_group_layer(ar, lib, c, DEEP) for c in layers]
    arr = (_lib.LayerArgs * 2)(*[b["args"] for b in bufs])
    ar.fill(0xFF)
    seq = E._kernel_seq(lambda: (_lib.check(lib.sow_forward_group(arr, 2, _lib.BF16 | DEEP, E._stream()), "sow_forward_group"),
                                 _lib.check(lib.sow_backward_group(arr, 2, _lib.BF16 | DEEP, _lib.BWD_DATA | _lib.BWD_WEIGHTS,
                                                                   E._stream()), "sow_backward_group")))
    ar.check_guards("group of two")
    assert sum(KERNEL in k for k in seq) == 4, seq
    for c, b, s in zip(layers, bufs, singles):
        _same_bits(s, _got(b), c.name + ": group of two vs single", keys=("y", "h", "dx", "dA", "dB", "dbias"))


def test_mixed_group_partitions_by_permission():
    """ops.LayerGroup over a deep layer, a SOW_FUSE_ACC layer and an unflagged layer: one C call per permission value for the
    forward and the data gradient, every layer with the bits of its single call."""
    from sow_amd import ops
    layers = [(DA.BY_NAME["tot258"], DEEP), (FA.CASES[1], FUSE), (FA.CASES[0], 0)]
    singles = [_run(c, _data(c), flags=f) for c, f in layers]
    calls, keep = [], []
    for c, f in layers:
        d = {k: (None if v is None else v.to(DEV)) for k, v in _data(c).items()}
        out = (torch.empty(c.d_in, c.r, dtype=BF16, device=DEV), torch.empty(c.r, c.d_out, dtype=BF16, device=DEV),
               torch.empty(c.d_out, dtype=BF16, device=DEV) if c.bias else None)
        dx = torch.empty(c.T, c.d_in, dtype=BF16, device=DEV)
        calls.append(ops.LayerCall(d["x"], d["A"], d["B"], acc_down=d["Q"], acc_up=d["R"], bias=d.get("bias"), scale=c.s,
                                   dy2=d["dy"], dx=dx, out=out, fuse_acc=f if f else False))
        keep.append((d, out, dx))
    g = ops.LayerGroup(calls)
    assert g._perms == [DEEP, FUSE, 0] and [dt for _, _, dt in g._by_permission()] == [_lib.BF16 | FUSE, _lib.BF16 | DEEP, _lib.BF16]
    seq = E._kernel_seq(lambda: (g.forward(), g.backward()))
    assert sum(KERNEL in k for k in seq) == 2 and sum("chain_wide_acc_kernel" in k for k in seq) == 2, seq
    for (c, f), call, (d, out, dx), s in zip(layers, calls, keep, singles):
        got = dict(y=call.y.cpu(), h=call.h.view(c.T, 64).cpu(), dx=dx.cpu(), dA=out[0].cpu(), dB=out[1].cpu(),
                   dbias=None if out[2] is None else out[2].cpu())
        _same_bits(s, got, c.name + ": mixed group vs single", keys=("y", "h", "dx", "dA", "dB", "dbias"))


# ---- permission semantics
BASE = DA.BY_NAME["tot258"]
PERMISSION = {
    "total_962": dict(c=DA.case("total_962", BF16, 65, 72, 136, 52, 910)),
    "r_live_66": dict(c=DA.case("r_live_66", BF16, 193, 72, 264, 66, 250)),
    "odd_r_acc": dict(c=DA.case("odd_r_acc", BF16, 193, 72, 264, 50, 251)),
    "d_out_not_mod_8": dict(c=DA.case("d_out_268", BF16, 193, 72, 268, 58, 200)),
    "param_f32": dict(c=BASE, flags=_lib.PARAM_F32, param_f32=True),
    "switch_NO_DEEP_ACC": dict(c=dataclasses.replace(BASE, switches=dict(NO_DEEP_ACC=1))),
    "unflagged_workspace": dict(c=BASE, ws_flags=0),
}


@pytest.mark.parametrize("name", list(PERMISSION))
def test_flag_is_a_permission(name):
    """A flagged call outside the admitted set (or without the flagged workspace, or with the switch) returns SOW_OK -- the
    runner checks every return code -- and gives the bits of the unflagged call."""
    p = PERMISSION[name]
    c, extra = p["c"], p.get("flags", 0)
    d = _data(c)
    pf = p.get("param_f32", False)
    plain = _run(c, d, flags=extra, param_f32=pf)
    trace = {}
    flagged = _run(c, d, flags=extra | DEEP, ws_flags=p.get("ws_flags", extra | DEEP), trace=trace, param_f32=pf)
    _no_deep(trace, name)
    _same_bits(plain, flagged, name)


def test_unflagged_workspace_is_smaller_for_the_permission_case():
    """The premise of the `unflagged_workspace` case: the flagged plan of that shape is larger than the unflagged one."""
    lib = _lib.load()
    c = BASE
    args = (c.T, c.d_in, c.d_out, c.r, c.r_acc, _lib.ACC_LOWRANK)
    assert lib.sow_workspace_bytes(*args, _lib.BF16 | DEEP) > lib.sow_workspace_bytes(*args, _lib.BF16)
    assert lib.sow_forward_workspace_bytes(*args, _lib.BF16 | DEEP) > lib.sow_forward_workspace_bytes(*args, _lib.BF16)


def test_both_bits_below_257_columns_run_the_fused_pass():
    """SOW_FUSE_ACC | SOW_FUSE_ACC_DEEP on a layer of total 100: the bits and the trace of SOW_FUSE_ACC alone."""
    c = FA.CASES[0]
    d = _data(c)
    t1, t2 = {}, {}
    one = _run(c, d, flags=FUSE, trace=t1)
    both = _run(c, d, flags=FUSE | DEEP, trace=t2)
    assert t1 == t2 and any("chain_wide_acc_kernel" in k for k in t2["fwd"]) and not any(KERNEL in k for k in t2["fwd"] + t2["bwd"])
    _same_bits(one, both, "both bits")


# ---- containment
def test_nan_in_x_stays_in_its_row():
    c = BASE
    d = dict(_data(c))
    clean = _run(c, d, flags=DEEP, backward=False)
    d["x"] = d["x"].clone()
    d["x"][1, 37] = float("nan")
    out = _run(c, d, flags=DEEP, backward=False)
    y, h = out["y"].float(), out["h"].float()
    assert torch.isnan(y[1]).all() and torch.isnan(h[1, :c.r]).all()
    assert (h[1, c.r:63] == 0).all() and h[1, 63] == 1.0          # the padding of the row stays the contract's
    rows = torch.arange(c.T) != 1
    assert not torch.isnan(y[rows]).any() and not torch.isnan(h[rows]).any()
    assert torch.equal(E._bits(out["y"][rows]), E._bits(clean["y"][rows]))
    assert torch.equal(E._bits(out["h"][rows]), E._bits(clean["h"][rows]))


@pytest.mark.parametrize("c", [DA.BY_NAME["straddle_256"], DA.BY_NAME["tot320_r64"]], ids=lambda c: c.name)
def test_exact_small_integer_operands(c):
    """Operands of tests/value_plan.py (small integers, every intermediate representable, every sum below 2^24 units): h_save,
    y, dX and the weight gradients equal the exact result bit for bit."""
    lay = FP.Layer(name=c.name, dtype={BF16: "bf16", F16: "f16"}[c.dtype], T=c.T, d_in=c.d_in, d_out=c.d_out, r=c.r, acc="lowrank",
                   r_acc=c.r_acc, bias=c.bias, s=0.5)
    d, f = V.exact_layer_proved(lay)
    cc = dataclasses.replace(c, s=0.5)
    trace = {}
    out = _run(cc, {k: (None if v is None else v.to(c.dtype)) for k, v in d.items()}, flags=DEEP, trace=trace)
    _deep_trace(trace, c.name)
    for k in ("y", "dx", "dA", "dB") + (("dbias",) if c.bias else ()):
        check_rounded(out[k], f[k], c.dtype, max_ulp=0, max_inexact=0, min_count=0, name=f"{c.name}: exact {k}")
        assert torch.equal(E._bits(out[k] + 0), E._bits(rne(f[k], c.dtype).to(c.dtype) + 0)), f"{c.name}: {k} bits"
    for k, ref in (("h", f["h"]), ("dh", f["dh"])):
        assert torch.equal(out[k][:, :c.r].double(), ref), f"{c.name}: exact {k}"


# ---- module level: a layer pretrained from scratch, through every stage of its accumulator
def test_module_through_every_accumulator_stage(monkeypatch):
    from conftest import rel_err
    from oracle import sow_oracle as O
    from sow_amd import ops
    from sow_amd.layer import SoWLinear
    monkeypatch.setattr(ops, "fused_acc_pays", lambda *a: True)
    monkeypatch.setattr(ops, "deep_acc_pays", lambda *a: True)
    g = torch.Generator().manual_seed(777)
    T, d_in, d_out, r, scale = 130, 320, 328, 50, 0.75
    layer = SoWLinear(d_in, d_out, bias=True, rank=r, scale=scale, init_method="normal", device=DEV, dtype=BF16)
    x = torch.randn(T, d_in, generator=g).to(BF16).to(DEV).requires_grad_(True)
    dy = torch.randn(T, d_out, generator=g).to(BF16).to(DEV)
    f = lambda t: t.detach().float().cpu()
    tol = 2e-2          # tests/test_gpu_parity.py: bf16 against the fp32 oracle

    def step():
        layer.zero_grad()
        x.grad = None
        y = layer(x)
        y.backward(dy)
        return y

    stages = []
    for stage in range(7):
        with torch.no_grad():   # accumulate() zeroes B: give the live term something to carry
            layer.upscale_weights[0].copy_((torch.randn(r, d_out, generator=g) * 0.05).to(BF16))
            layer.downscale_weights[0].copy_((torch.randn(d_in, r, generator=g) * 0.05).to(BF16))
            layer.bias.copy_((torch.randn(d_out, generator=g) * 0.1).to(BF16))
        layer.accumulate()
        with torch.no_grad():
            layer.upscale_weights[0].copy_((torch.randn(r, d_out, generator=g) * 0.05).to(BF16))
        lowrank = layer.acc_upweight.numel() != 0
        r_acc = layer.acc_downweight.shape[1] if lowrank else None
        stages.append(r_acc)
        holder = {}
        seq = E._kernel_seq(lambda: holder.update(y=step()))
        y = holder["y"]
        n_fused, n_deep = sum("chain_wide_acc_kernel" in k for k in seq), sum(KERNEL in k for k in seq)
        want = (2, 0) if lowrank and r_acc + r <= 256 else (0, 2) if lowrank else (0, 0)
        assert (n_fused, n_deep) == want, (stage, r_acc, seq)
        with torch.no_grad():
            y_eval = layer(x)
        assert torch.equal(E._bits(y_eval), E._bits(y.detach())), f"stage {stage}: eval and train forward differ"
        A, B, b = f(layer.downscale_weights[0]), f(layer.upscale_weights[0]), f(layer.bias)
        Q, R = f(layer.acc_downweight), (f(layer.acc_upweight) if lowrank else None)
        y_ref = O.sow_forward(f(x), [A], [B], Q, R, scale, b)
        dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(f(dy), f(x), [A], [B], Q, R, scale, True)
        errs = dict(y=rel_err(f(y), y_ref), dx=rel_err(f(x.grad), dx_ref), dA=rel_err(f(layer.downscale_weights[0].grad), dA_ref[0]),
                    dB=rel_err(f(layer.upscale_weights[0].grad), dB_ref[0]), dbias=rel_err(f(layer.bias.grad), db_ref))
        print(f"stage {stage} r_acc {r_acc}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) < tol, (stage, r_acc, errs)
    assert stages == [50, 100, 150, 200, 250, 300, None], stages


def test_zz_report_worst_ratios():
    for (case, stage), w in sorted(WORST.items()):
        print(f"worst err/limit {case:18s} {stage:7s} {w:.3f}")
