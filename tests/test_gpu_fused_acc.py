"""-m gpu: the fused low-rank-accumulator pass (SOW_FUSE_ACC, chain_wide_acc.hip) through the C ABI, element by element
against float64 (tests/fused_acc_numerics.py), on NaN-poisoned memory -- and the permission semantics of the flag: every
flagged call outside the admitted set gives the bits of the unflagged call.

The runner is test_gpu_elementwise's (guarded views with NaN neighbours, sentinel guards around every output, outputs and
workspaces poisoned / zeroed / poisoned, three bit-identical runs) with the dtype of the calls and of the workspace queries
chosen separately.
"""
import dataclasses

import pytest
import torch

import fused_acc_numerics as FA
import fuzz_plan as FP
import test_gpu_elementwise as E
import value_plan as V
from numerics import check_h_save, check_rounded, fp32_floor, rne, to64
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
FUSE = _lib.FUSE_ACC
WORST = {}
_DATA = {}
TWO_PASS = ("chain2", "chain_kernel", "chain_wide_kernel", "gemm")   # today's kernels that write y / dX


def _data(c):
    if c.name not in _DATA:
        _DATA[c.name] = E._inputs(c)
    return _DATA[c.name]


def _run(c, d, flags=FUSE, ws_flags=None, trace=None, save_h=True, backward=True, param_f32=False, group=False):
    """Forward (+ backward) of layer c through the C ABI with `flags` OR-ed into the dtype of the calls and `ws_flags`
    (default: the same) into the dtype of the workspace queries; three runs (poisoned, zeroed, poisoned) that must agree bit
    for bit.  Returns the outputs of the first run on the CPU, with "dh": the [T, 64] dh region of the backward workspace.
    param_f32: fp32 A, B, bias, Q, R and gradients (SOW_PARAM_F32 must then be in `flags`).  group: through
    sow_forward_group / sow_backward_group as a group of one."""
    with _lib.switch(**c.switches):
        return _run_switched(c, d, flags, flags if ws_flags is None else ws_flags, trace, save_h, backward, param_f32, group)


def _run_switched(c, d, flags, ws_flags, trace, save_h, backward, param_f32, group):
    lib = _lib.load()
    dt, qdt, kind = E._dt(c.dtype) | flags, E._dt(c.dtype) | ws_flags, _lib.ACC_LOWRANK
    ar = E.Arena(c.dtype)
    par = E.Arena(F32) if param_f32 else ar
    x, dy = ar.input(d["x"]), ar.input(d["dy"])
    A, B, bias, Q, R = (par.input(d.get(k)) for k in ("A", "B", "bias", "Q", "R"))
    hcols = 64 if c.r <= 64 else c.r
    y = ar.output((c.T, c.d_out))
    h = ar.output((c.T, hcols), misalign=0) if save_h else None
    fws = ar.workspace(lib.sow_forward_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, qdt))
    backward = backward and save_h
    if backward:
        h_in = ar.input(torch.zeros(c.T, hcols), misalign=0)
        dx = ar.output((c.T, c.d_in))
        dA, dB = par.output((c.d_in, c.r), misalign=0), par.output((c.r, c.d_out), misalign=0)
        dbias = par.output((c.d_out,), misalign=0) if c.bias else None
        bws = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, qdt))
    arr = (_lib.LayerArgs * 1)()

    def layer_args(fwd_call):
        ws = fws if fwd_call else bws
        return _lib.LayerArgs(x=E._ptr(x), A=E._ptr(A), B=E._ptr(B), acc_down=E._ptr(Q), acc_up=E._ptr(R), bias=E._ptr(bias),
                              y=E._ptr(y), h_save=E._ptr(h if fwd_call else h_in), dy=E._ptr(dy),
                              dx=E._ptr(dx) if backward else None, dA=E._ptr(dA) if backward else None,
                              dB=E._ptr(dB) if backward else None, dbias=E._ptr(dbias) if backward else None, T=c.T,
                              d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=c.r_acc, acc_kind=kind, scale=c.s, grad_beta=0.0,
                              workspace=E._ptr(ws), workspace_bytes=0 if ws is None else ws.numel())

    def fwd():
        if group:
            arr[0] = layer_args(True)
            return _lib.check(lib.sow_forward_group(arr, 1, dt, E._stream()), "sow_forward_group")
        _lib.check(lib.sow_forward(E._ptr(x), E._ptr(A), E._ptr(B), E._ptr(Q), E._ptr(R), E._ptr(bias), E._ptr(y), E._ptr(h),
                                   c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, c.s, dt, E._ptr(fws),
                                   0 if fws is None else fws.numel(), E._stream()), "sow_forward")

    def bwd_call():
        if group:
            arr[0] = layer_args(False)
            return _lib.check(lib.sow_backward_group(arr, 1, dt, _lib.BWD_DATA | _lib.BWD_WEIGHTS, E._stream()),
                              "sow_backward_group")
        _lib.check(lib.sow_backward_ex(E._ptr(dy), E._ptr(x), E._ptr(h_in), E._ptr(A), E._ptr(B), E._ptr(Q), E._ptr(R),
                                       E._ptr(dx), E._ptr(dA), E._ptr(dB), E._ptr(dbias), c.T, c.d_in, c.d_out, c.r, c.r_acc,
                                       kind, c.s, 0.0, dt, E._ptr(bws), bws.numel(), _lib.BWD_DATA | _lib.BWD_WEIGHTS,
                                       E._stream()), "sow_backward_ex")

    def dh_region():
        """The first T x 64 elements of the 256-byte-aligned backward workspace: dh of an r_live <= 64 layer."""
        off = (-bws.data_ptr()) % 256
        return bws[off:off + c.T * 64 * 2].view(c.dtype).view(c.T, 64).clone()

    runs = []
    for byte in (0xFF, 0x00, 0xFF):
        ar.fill(byte)
        if par is not ar:
            par.fill(byte)
        profiled = trace is not None and len(runs) == 2
        if profiled:
            trace["fwd"] = E._kernel_seq(fwd)
        else:
            fwd()
        outs = dict(y=y.clone(), h=None if h is None else h.clone())
        if backward:
            h_in.copy_(h)
            if profiled:
                trace["bwd"] = E._kernel_seq(bwd_call)
            else:
                bwd_call()
            outs.update(dx=dx.clone(), dA=dA.clone(), dB=dB.clone(), dbias=None if dbias is None else dbias.clone())
            if c.r <= 64:
                outs["dh"] = dh_region()
        ar.check_guards(f"{c.name} run {len(runs)}")
        if par is not ar:
            par.check_guards(f"{c.name} run {len(runs)} (fp32 parameters)")
        runs.append(outs)
    for k, v in runs[0].items():
        if v is None:
            continue
        for i in (1, 2):
            assert torch.equal(E._bits(v), E._bits(runs[i][k])), \
                f"{c.name}: {k} of the {'zeroed' if i == 1 else 'repeated'} run differs from the poisoned run"
    return {k: (None if v is None else v.cpu()) for k, v in runs[0].items()}


def _same_bits(a, b, what, keys=("y", "h", "dx", "dA", "dB", "dbias", "dh")):
    for k in keys:
        if a.get(k) is None and b.get(k) is None:
            continue
        assert torch.equal(E._bits(a[k]), E._bits(b[k])), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} elements"


def _fused_trace(trace, name):
    for ph in ("fwd", "bwd"):
        seq = trace[ph]
        assert sum("chain_wide_acc_kernel" in k for k in seq) == 1, f"{name} {ph}: no fused launch in {seq}"
        bad = [k for k in seq if any(t in k for t in TWO_PASS) and "chain_wide_acc_kernel" not in k]
        assert not bad, f"{name} {ph}: two-pass kernels next to the fused one: {bad}"
    assert "wide_acc_pack_kernel" in trace["fwd"][0] and "wide_acc_pack_kernel" in trace["bwd"][0]


def _two_pass_trace(trace, name):
    for ph in ("fwd", "bwd"):
        seq = trace[ph]
        assert not any("wide_acc" in k for k in seq), f"{name} {ph}: a fused launch in {seq}"
        assert sum(any(t in k for t in TWO_PASS) for k in seq) >= 2, f"{name} {ph}: fewer than two chain launches in {seq}"


# ---- 1, 2, 3a, 5b: element-wise against float64, trace, determinism, no poison left
@pytest.mark.parametrize("c", FA.CASES, ids=lambda c: c.name)
def test_fused_layer_elementwise(c):
    d = _data(c)
    trace = {}
    out = _run(c, d, trace=trace)
    _fused_trace(trace, c.name)
    worst = FA.check(c, d, out)
    WORST.update({(c.name, k): v for k, v in worst.items()})
    # dh, which the weight kernels read: the r <= 64 contract, every byte written
    dy, B = to64(d["dy"]), to64(d["B"])
    ref = c.s * (dy @ B.t())
    st = check_h_save(to64(out["dh"]), ref, c.r, c.dtype, acc=fp32_floor(c.s * c.s * ((dy * dy) @ (B * B).t()), c.d_out),
                      name=f"{c.name}: dh")
    WORST[(c.name, "dh")] = st["worst"]
    for k in ("y", "h", "dx", "dA", "dB", "dbias"):
        assert out[k] is None or not torch.isnan(out[k].float()).any(), f"{c.name}: poison left in {k}"


UNFLAGGED = [FA.CASES[0], FA.CASES[1], FA.CASES[4]]   # chain2 + chain2, chain_wide + chain2, the generic chain twice


@pytest.mark.parametrize("c", UNFLAGGED, ids=lambda c: c.name)
def test_unflagged_call_runs_the_two_pass_kernels(c):
    """The same call without the flag: today's kernels, repeatable bits (the three runs of the runner), and outputs inside
    the two-pass bound of test_gpu_elementwise."""
    d = _data(c)
    trace = {}
    out = _run(c, d, flags=0, trace=trace)
    _two_pass_trace(trace, c.name)
    E._check(dataclasses.replace(c, y_rounds="twice"), d, {k: v for k, v in out.items() if k != "dh"})


# ---- 3b: grouped entry points, h_save = NULL
@pytest.mark.parametrize("c", [FA.CASES[0], FA.CASES[2]], ids=lambda c: c.name)
def test_group_fall_through_gives_the_bits_of_the_single_call(c):
    d = _data(c)
    single = _run(c, d)
    trace = {}
    grouped = _run(c, d, group=True, trace=trace)
    _fused_trace(trace, c.name + " (group)")
    _same_bits(single, grouped, c.name + ": group vs single")


def test_group_of_two_flagged_layers():
    """sow_forward_group / sow_backward_group of two flagged layers: each layer gets the bits of its single call."""
    lib = _lib.load()
    layers = [FA.CASES[0], FA.CASES[1]]
    singles = [_run(c, _data(c)) for c in layers]
    ar = E.Arena(BF16)
    arr = (_lib.LayerArgs * 2)()
    bufs = []
    for i, c in enumerate(layers):
        d = _data(c)
        b = {k: ar.input(d.get(k)) for k in ("x", "A", "B", "bias", "dy", "Q", "R")}
        b.update(y=ar.output((c.T, c.d_out)), h=ar.output((c.T, 64)), dx=ar.output((c.T, c.d_in)), dA=ar.output((c.d_in, c.r)),
                 dB=ar.output((c.r, c.d_out)), dbias=ar.output((c.d_out,)) if c.bias else None)
        b["ws"] = ar.workspace(lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, _lib.ACC_LOWRANK, _lib.BF16 | FUSE))
        bufs.append(b)
        arr[i] = _lib.LayerArgs(x=E._ptr(b["x"]), A=E._ptr(b["A"]), B=E._ptr(b["B"]), acc_down=E._ptr(b["Q"]), acc_up=E._ptr(b["R"]),
                                bias=E._ptr(b["bias"]), y=E._ptr(b["y"]), h_save=E._ptr(b["h"]), dy=E._ptr(b["dy"]),
                                dx=E._ptr(b["dx"]), dA=E._ptr(b["dA"]), dB=E._ptr(b["dB"]), dbias=E._ptr(b["dbias"]), T=c.T,
                                d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=c.r_acc, acc_kind=_lib.ACC_LOWRANK, scale=c.s,
                                grad_beta=0.0, workspace=E._ptr(b["ws"]), workspace_bytes=b["ws"].numel())
    ar.fill(0xFF)
    seq = E._kernel_seq(lambda: (_lib.check(lib.sow_forward_group(arr, 2, _lib.BF16 | FUSE, E._stream()), "sow_forward_group"),
                                 _lib.check(lib.sow_backward_group(arr, 2, _lib.BF16 | FUSE, _lib.BWD_DATA | _lib.BWD_WEIGHTS,
                                                                   E._stream()), "sow_backward_group")))
    ar.check_guards("group of two")
    assert sum("chain_wide_acc_kernel" in k for k in seq) == 4, seq
    for c, b, s in zip(layers, bufs, singles):
        got = {k: (None if b[k] is None else b[k].cpu()) for k in ("y", "h", "dx", "dA", "dB", "dbias")}
        _same_bits(s, got, c.name + ": group of two vs single", keys=("y", "h", "dx", "dA", "dB", "dbias"))


@pytest.mark.parametrize("c", [FA.CASES[0], FA.CASES[3]], ids=lambda c: c.name)
def test_h_save_null_gives_the_same_y(c):
    d = _data(c)
    with_h = _run(c, d, backward=False)
    trace = {}
    without = _run(c, d, save_h=False, trace=trace)
    assert any("chain_wide_acc_kernel" in k for k in trace["fwd"])
    _same_bits(with_h, without, c.name + ": h_save = NULL", keys=("y",))
    FA.check(c, d, dict(y=without["y"]))


# ---- 4: permission semantics
BASE = FA.CASES[0]
PERMISSION = {
    "total_258": dict(c=FA.case("total_258", BF16, 193, 72, 264, 58, 200)),
    "r_live_66": dict(c=FA.case("r_live_66", BF16, 193, 72, 264, 66, 50)),
    "d_out_not_mod_8": dict(c=FA.case("d_out_268", BF16, 193, 72, 268, 50, 50)),
    "param_f32": dict(c=BASE, flags=_lib.PARAM_F32, param_f32=True),
    "switch_NO_FUSED_ACC": dict(c=dataclasses.replace(BASE, switches=dict(NO_FUSED_ACC=1))),
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
    flagged = _run(c, d, flags=extra | FUSE, ws_flags=p.get("ws_flags", extra | FUSE), trace=trace, param_f32=pf)
    assert not any("wide_acc" in k for k in trace["fwd"] + trace["bwd"]), f"{name}: a fused launch in {trace}"
    _same_bits(plain, flagged, name)


def test_unflagged_workspace_is_smaller_for_the_permission_case():
    """The premise of the `unflagged_workspace` case: the flagged plan of that shape is larger than the unflagged one."""
    lib = _lib.load()
    c = BASE
    args = (c.T, c.d_in, c.d_out, c.r, c.r_acc, _lib.ACC_LOWRANK)
    assert lib.sow_workspace_bytes(*args, _lib.BF16 | FUSE) > lib.sow_workspace_bytes(*args, _lib.BF16)
    assert lib.sow_forward_workspace_bytes(*args, _lib.BF16 | FUSE) > lib.sow_forward_workspace_bytes(*args, _lib.BF16)


# ---- 5: containment
def test_nan_in_x_stays_in_its_row():
    c = FA.CASES[0]
    d = dict(_data(c))
    clean = _run(c, d, backward=False)
    d["x"] = d["x"].clone()
    d["x"][1, 37] = float("nan")
    out = _run(c, d, backward=False)
    y, h = out["y"].float(), out["h"].float()
    assert torch.isnan(y[1]).all() and torch.isnan(h[1, :c.r]).all()
    assert (h[1, c.r:63] == 0).all() and h[1, 63] == 1.0          # the padding of the row stays the contract's
    rows = torch.arange(c.T) != 1
    assert not torch.isnan(y[rows]).any() and not torch.isnan(h[rows]).any()
    assert torch.equal(E._bits(out["y"][rows]), E._bits(clean["y"][rows]))
    assert torch.equal(E._bits(out["h"][rows]), E._bits(clean["h"][rows]))


@pytest.mark.parametrize("c", [FA.CASES[0], FA.CASES[3]], ids=lambda c: c.name)
def test_exact_small_integer_operands(c):
    """Operands of tests/value_plan.py (small integers, every intermediate representable, every sum below 2^24 units): h_save,
    y, dX and the weight gradients equal the exact result bit for bit."""
    lay = FP.Layer(name=c.name, dtype={BF16: "bf16", F16: "f16"}[c.dtype], T=c.T, d_in=c.d_in, d_out=c.d_out, r=c.r, acc="lowrank",
                   r_acc=c.r_acc, bias=c.bias, s=0.5)
    d, f = V.exact_layer_proved(lay)
    cc = dataclasses.replace(c, s=0.5)
    trace = {}
    out = _run(cc, {k: (None if v is None else v.to(c.dtype)) for k, v in d.items()}, trace=trace)
    _fused_trace(trace, c.name)
    for k in ("y", "dx", "dA", "dB") + (("dbias",) if c.bias else ()):
        check_rounded(out[k], f[k], c.dtype, max_ulp=0, max_inexact=0, min_count=0, name=f"{c.name}: exact {k}")
        assert torch.equal(E._bits(out[k] + 0), E._bits(rne(f[k], c.dtype).to(c.dtype) + 0)), f"{c.name}: {k} bits"
    for k, ref in (("h", f["h"]), ("dh", f["dh"])):
        assert torch.equal(out[k][:, :c.r].double(), ref), f"{c.name}: exact {k}"


# ---- 6: module level
def test_module_forward_backward_against_the_oracle(monkeypatch):
    from conftest import rel_err
    from oracle import sow_oracle as O
    from sow_amd import ops
    from sow_amd.layer import SoWLinear
    import torch.nn as nn
    monkeypatch.setattr(ops, "fused_acc_pays", lambda *a: True)
    g = torch.Generator().manual_seed(4242)
    T, d_in, d_out, r, r_acc, scale = 300, 512, 264, 50, 100, 0.75
    layer = SoWLinear(d_in, d_out, bias=True, rank=r, scale=scale, init_method="normal", device=DEV, dtype=BF16)
    Q, R = (torch.randn(d_in, r_acc, generator=g) * 0.1).to(BF16), (torch.randn(r_acc, d_out, generator=g) * 0.1).to(BF16)
    layer.acc_downweight = nn.Parameter(Q.to(DEV), requires_grad=False)
    layer.acc_upweight = nn.Parameter(R.to(DEV), requires_grad=False)
    with torch.no_grad():
        layer.upscale_weights[0].copy_((torch.randn(r, d_out, generator=g) * 0.02).to(BF16))
        layer.bias.copy_((torch.randn(d_out, generator=g) * 0.1).to(BF16))
    x = torch.randn(T, d_in, generator=g).to(BF16).to(DEV).requires_grad_(True)
    dy = torch.randn(T, d_out, generator=g).to(BF16).to(DEV)

    def step():
        layer.zero_grad()
        x.grad = None
        y = layer(x)
        y.backward(dy)
        return y

    step()
    y = None
    seq = E._kernel_seq(lambda: step())
    y = layer(x)
    assert sum("chain_wide_acc_kernel" in k for k in seq) == 2, seq
    assert not any(any(t in k for t in TWO_PASS) and "wide_acc" not in k for k in seq), seq
    with torch.no_grad():
        y_eval = layer(x)
    assert torch.equal(E._bits(y_eval), E._bits(y.detach())), "eval and train forward differ"
    f = lambda t: t.detach().float().cpu()
    A, B, b = f(layer.downscale_weights[0]), f(layer.upscale_weights[0]), f(layer.bias)
    y_ref = O.sow_forward(f(x), [A], [B], f(Q), f(R), scale, b)
    dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(f(dy), f(x), [A], [B], f(Q), f(R), scale, True)
    tol = 2e-2          # tests/test_gpu_parity.py: bf16 against the fp32 oracle
    assert rel_err(f(y), y_ref) < tol and rel_err(f(x.grad), dx_ref) < tol
    assert rel_err(f(layer.downscale_weights[0].grad), dA_ref[0]) < tol
    assert rel_err(f(layer.upscale_weights[0].grad), dB_ref[0]) < tol
    assert rel_err(f(layer.bias.grad), db_ref) < tol


def test_zz_report_worst_ratios():
    for (case, stage), w in sorted(WORST.items()):
        print(f"worst err/limit {case:16s} {stage:7s} {w:.3f}")
