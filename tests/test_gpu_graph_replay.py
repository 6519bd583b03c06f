"""-m gpu: every entry point of the C ABI and the Python training step, captured into a HIP graph and replayed in place.

The cases are those of tests/graph_plan.py (one per kernel family), the protocol that of tests/graph_replay.py: eager twins
on two input sets, a warm-up on a side stream, a linear capture on that stream that must run nothing, and three replays --
on the captured inputs, on inputs changed in place over zeroed workspaces, and on the leftovers of the second -- that must
reproduce the eager twins bit for bit.  The second replay is also checked against float64 with the checker and the bounds of
the case's home module (numerics.py, step_numerics.py, tt_numerics.py, fused_acc_numerics.py, grad_stats_ref.py ...); no
tolerance is introduced here.  The eager twin of every case is traced, and test_zz_graph_coverage (last) asserts that every
kernel the plan claims appeared and that claims and exemptions cover every __global__ of the sources.

test_step_* capture the Python training step (SoWLinear siblings behind FactorBucket.attach, FactorAdamW.step with a device
loss scale, clipping and skip_nonfinite, bucket.zero_grad()) and replay it on a finite batch, an overflowing one and a
finite one against an eager twin.
"""
import ctypes
import dataclasses
import math
import struct
import types

import pytest
import torch
import torch.nn as nn

import fused_acc_numerics as FA
import graph_plan as GP
import graph_replay as GR
import grad_stats_ref as R
import shared_fused_acc_numerics as SN
import test_gpu_elementwise as E
import test_gpu_shared_input as SI
import test_gpu_skinny as SK
import test_gpu_step_elementwise as SE
import test_gpu_tt_elementwise as TTE
import tt_numerics as T
from numerics import check_bound, fp32_floor, gemm_epilogue, gemm_f32_bound, rne, to64, ulp
from step_numerics import (U32, adamw_ref, check_qr, check_rank_update, check_rounded_noisy, check_step, ttadam_ref)
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {"bf16": BF16, "f16": F16, "f32": F32}
BETAS, EPS = (0.9, 0.999), 1e-8
SEED2 = 101                  # what the second input set adds to a case's seed
TRACES = {}                  # case id -> kernel names of its eager run on I1


def _p(t):
    return None if t is None else t.data_ptr()


def _half(d):
    """The second input set of a case: the tensors of another seed, scaled by 0.5 (exact in every dtype)."""
    if isinstance(d, dict):
        return {k: _half(v) for k, v in d.items()}
    if isinstance(d, (list, tuple)):
        return type(d)(_half(v) for v in d)
    return d * 0.5 if isinstance(d, torch.Tensor) and d.is_floating_point() else d


def _pair(I, k):
    a, b = I[0].get(k), I[1].get(k)
    return None if a is None else (a, b)


# ---------------------------------------------------------------------------------------------------------------- layers
def _e_case(lay, name=None):
    return E.Case(name or lay.name, DT[lay.dtype], lay.T, lay.d_in, lay.d_out, lay.r, acc=lay.acc, r_acc=lay.r_acc, bias=lay.bias,
                  s=lay.s, grad_beta=lay.grad_beta, misalign=lay.misalign, switches=dict(lay.switches), y_rounds=lay.y_rounds,
                  save_h=True, seed=lay.seed, dx_rounds=lay.dx_rounds)


def _layer_sets(c, param_f32=False):
    """The two input sets of a layer (test_gpu_elementwise._inputs).  param_f32: fp32 values for the parameters and the
    gradients accumulated onto (the library rounds them once to the compute dtype)."""
    cc = dataclasses.replace(c, dtype=F32) if param_f32 else c
    I = [E._inputs(cc), _half(E._inputs(dataclasses.replace(cc, seed=c.seed + SEED2)))]
    if param_f32:
        for d in I:
            d["x"], d["dy"] = d["x"].to(c.dtype), d["dy"].to(c.dtype)
    return I


def build_layer(case):
    lib = _lib.load()
    p = case.p
    c = _e_case(p["layer"])
    pf = p["param_f32"]
    perm = getattr(_lib, p["flags"]) if p["flags"] else 0
    dt = E._dt(c.dtype) | perm | (_lib.PARAM_F32 if pf else 0)
    kind = E._kind(c)
    I = _layer_sets(c, pf)
    b = GR.Bound(case.id)
    ar = b.arena(c.dtype, c.misalign)
    par = b.arena(F32) if pf else ar
    x, dy = b.input(ar, _pair(I, "x")), b.input(ar, _pair(I, "dy"))
    A, B, bias = (b.input(par, _pair(I, k)) for k in ("A", "B", "bias"))
    acc_down = b.input(par, _pair(I, "W") or _pair(I, "Q"))
    acc_up = b.input(par, _pair(I, "R"))
    hcols = 64 if c.r <= 64 else c.r
    y = b.output(ar, "y", (c.T, c.d_out))
    h = b.output(ar, "h", (c.T, hcols), misalign=0)
    dx = b.output(ar, "dx", (c.T, c.d_in))
    dA = b.output(par, "dA", (c.d_in, c.r), _pair(I, "dA0"), misalign=0)
    dB = b.output(par, "dB", (c.r, c.d_out), _pair(I, "dB0"), misalign=0)
    dbias = b.output(par, "dbias", (c.d_out,), _pair(I, "dbias0"), misalign=0) if c.bias else None
    fws = b.workspace(ar, lib.sow_forward_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, dt))
    bws = b.workspace(ar, lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, dt))

    def call(rc):
        s = E._stream()
        rc(lib.sow_forward(_p(x), _p(A), _p(B), _p(acc_down), _p(acc_up), _p(bias), _p(y), _p(h), c.T, c.d_in, c.d_out, c.r,
                           c.r_acc, kind, c.s, dt, _p(fws), 0 if fws is None else fws.numel(), s), "sow_forward")
        rc(lib.sow_backward_ex(_p(dy), _p(x), _p(h), _p(A), _p(B), _p(acc_down), _p(acc_up), _p(dx), _p(dA), _p(dB), _p(dbias),
                               c.T, c.d_in, c.d_out, c.r, c.r_acc, kind, c.s, c.grad_beta, dt, _p(bws), bws.numel(),
                               _lib.BWD_DATA | _lib.BWD_WEIGHTS, s), "sow_backward_ex")

    def check(k, out):
        d = I[k]
        out = dict(out, dbias=out.get("dbias"))
        if p["check"] == "fused":
            FA.check(c, d, out)
        elif p["check"] == "param_f32":
            # the flagged call is the plain call on the parameters rounded once (test_gpu_autocast.py): y, h_save and dX
            # against float64 as they are, the fp32 gradients rounded to the compute dtype -- and dB, dbias, whose operands
            # the test sees, within the fp32 bound of test_gpu_autocast.test_fp32_gradients_against_float64
            seen = {n: (None if v is None else v.to(c.dtype)) for n, v in d.items()}
            E._check(c, seen, {n: (None if v is None else v.to(c.dtype)) for n, v in out.items()})
            hh, dyy = to64(out["h"])[:, :c.r], to64(seen["dy"])
            new = hh.t() @ dyy
            check_bound(out["dB"], new, 2 * ulp(new, F32) + fp32_floor((hh * hh).t() @ (dyy * dyy), c.T), name=f"{c.name}: fp32 dB")
            if c.bias:
                new = dyy.sum(0)
                check_bound(out["dbias"], new, 2 * ulp(new, F32) + fp32_floor((dyy * dyy).sum(0), c.T), name=f"{c.name}: fp32 dbias")
        else:
            E._check(c, d, out)

    b.call, b.check = call, check
    return b


# ---------------------------------------------------------------------------------------------------------------- groups
def build_group(case):
    lib = _lib.load()
    p = case.p
    layers = [_e_case(lay, name=f"{case.id}.{lay.name}") for lay in p["layers"]]
    dtype = DT[p["dtype"]]
    dt = E._dt(dtype)
    n = len(layers)
    sets = [[E._inputs(c), _half(E._inputs(dataclasses.replace(c, seed=c.seed + SEED2)))] for c in layers]
    b = GR.Bound(case.id)
    ar = b.arena(dtype)
    arr = (_lib.LayerArgs * n)()
    for i, (c, I) in enumerate(zip(layers, sets)):
        v = {k: b.input(ar, _pair(I, k)) for k in ("x", "A", "B", "bias", "dy")}
        v.update(y=b.output(ar, f"y{i}", (c.T, c.d_out)), h=b.output(ar, f"h{i}", (c.T, 64), misalign=0),
                 dx=b.output(ar, f"dx{i}", (c.T, c.d_in)), dA=b.output(ar, f"dA{i}", (c.d_in, c.r), misalign=0),
                 dB=b.output(ar, f"dB{i}", (c.r, c.d_out), misalign=0),
                 dbias=b.output(ar, f"dbias{i}", (c.d_out,), misalign=0) if c.bias else None)
        ws = b.workspace(ar, lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, _lib.ACC_NONE, dt))
        arr[i] = _lib.LayerArgs(x=_p(v["x"]), A=_p(v["A"]), B=_p(v["B"]), acc_down=None, acc_up=None, bias=_p(v["bias"]),
                                y=_p(v["y"]), h_save=_p(v["h"]), dy=_p(v["dy"]), dx=_p(v["dx"]), dA=_p(v["dA"]), dB=_p(v["dB"]),
                                dbias=_p(v["dbias"]), T=c.T, d_in=c.d_in, d_out=c.d_out, r_live=c.r, r_acc=0,
                                acc_kind=_lib.ACC_NONE, scale=c.s, grad_beta=0.0, workspace=_p(ws), workspace_bytes=ws.numel())
    deferred = p["deferred"]
    phases = (_lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS) if deferred else (_lib.BWD_DATA | _lib.BWD_WEIGHTS)
    slabs = (ctypes.c_int * (2 * n))()
    assert lib.sow_backward_group_plan(arr, n, dt, phases, slabs) == int(p["rows"]), "the plan of graph_plan.py is not the C plan"
    descs = starts = None
    total = 0
    if deferred:      # the descriptors are built once, on the host, from pointers and shapes (no value of the operands)
        size = lib.sow_reduce_desc_bytes()
        raw = ctypes.create_string_buffer(size * n)
        blocks = (ctypes.c_int * n)()
        _lib.check(lib.sow_backward_group_reduce_desc(arr, n, dt, phases, raw, blocks), "sow_backward_group_reduce_desc")
        descs = torch.frombuffer(bytearray(raw.raw), dtype=torch.uint8).to(DEV)
        st = []
        for k in range(n):
            st.append(total)
            total += blocks[k]
        starts = torch.tensor(st, dtype=torch.int32, device=DEV)
        b.keep += [descs, starts]

    def call(rc):
        s = E._stream()
        rc(lib.sow_forward_group(arr, n, dt, s), "sow_forward_group")
        rc(lib.sow_backward_group(arr, n, dt, phases, s), "sow_backward_group")
        if deferred:
            rc(lib.sow_reduce_batch(_p(descs), _p(starts), n, total, dt, s), "sow_reduce_batch")

    def check(k, out):
        for i, (c, I) in enumerate(zip(layers, sets)):
            E._check(c, I[k], {key: out.get(f"{key}{i}") for key in ("y", "h", "dx", "dA", "dB", "dbias")})

    b.call, b.check = call, check
    return b


# ---------------------------------------------------------------------------------------------------------------- shared input
def build_shared(case):
    lib = _lib.load()
    p = case.p
    dtype = DT[p["dtype"]]
    dt = E._dt(dtype)
    st = SI.Set(case.id, dtype, p["T"], p["d_in"], [SI.Sib(*sb) for sb in p["sibs"]], grad_beta=p["grad_beta"])
    n = len(st.sibs)

    def data(seed, scale):
        x, per, dx0 = SI._data(st, seed=seed)
        f = lambda t: None if t is None else (t * scale).to(dtype)   # noqa: E731
        return dict(x=f(x), dx0=f(dx0), per=[{k: f(v) for k, v in q.items()} for q in per])

    I = [data(0, 1.0), data(SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(dtype)
    x = b.input(ar, (I[0]["x"], I[1]["x"]))
    dx = b.output(ar, "dx", (st.T, st.d_in), (I[0]["dx0"], I[1]["dx0"]))
    arr = (_lib.LayerArgs * n)()
    for i, sb in enumerate(st.sibs):
        q = [I[0]["per"][i], I[1]["per"][i]]
        v = {k: b.input(ar, _pair(q, k)) for k in ("A", "B", "bias", "dy")}
        zeros = (lambda *s: (torch.zeros(*s), torch.zeros(*s))) if (st.grad_beta and i == 0) else (lambda *s: None)
        y, h = b.output(ar, f"y{i}", (st.T, sb.d_out)), b.output(ar, f"h{i}", (st.T, 64))
        dA, dB = b.output(ar, f"dA{i}", (st.d_in, sb.r), zeros(st.d_in, sb.r)), b.output(ar, f"dB{i}", (sb.r, sb.d_out), zeros(sb.r, sb.d_out))
        dbias = b.output(ar, f"dbias{i}", (sb.d_out,), zeros(sb.d_out)) if sb.bias else None
        ws = b.workspace(ar, lib.sow_workspace_bytes(st.T, st.d_in, sb.d_out, sb.r, 0, _lib.ACC_NONE, dt))
        arr[i] = _lib.LayerArgs(x=_p(x), A=_p(v["A"]), B=_p(v["B"]), acc_down=None, acc_up=None, bias=_p(v["bias"]), y=_p(y),
                                h_save=_p(h), dy=_p(v["dy"]), dx=_p(dx) if i == 0 else None, dA=_p(dA), dB=_p(dB), dbias=_p(dbias),
                                T=st.T, d_in=st.d_in, d_out=sb.d_out, r_live=sb.r, r_acc=0, acc_kind=_lib.ACC_NONE, scale=sb.s,
                                grad_beta=st.grad_beta if i == 0 else 0.0, workspace=_p(ws), workspace_bytes=ws.numel())

    def call(rc):
        s = E._stream()
        rc(lib.sow_forward_shared(arr, n, dt, s), "sow_forward_shared")
        rc(lib.sow_backward_shared(arr, n, dt, _lib.BWD_DATA | _lib.BWD_WEIGHTS, s), "sow_backward_shared")

    def check(k, out):
        d = I[k]
        for i, sb in enumerate(st.sibs):
            c = E.Case(f"{case.id}.s{i}", dtype, st.T, st.d_in, sb.d_out, sb.r, bias=sb.bias, s=sb.s)
            q = d["per"][i]
            E._check(c, dict(x=d["x"], A=q["A"], B=q["B"], bias=q["bias"], dy=q["dy"]),
                     {key: out.get(f"{key}{i}") for key in ("y", "h", "dA", "dB", "dbias")})
        ref, bnd = SI._dx_reference(st, types.SimpleNamespace(inp=d["per"]), d["dx0"])
        check_bound(out["dx"], ref, bnd, name=f"{case.id}: dX")

    b.call, b.check = call, check
    return b


def build_shared_acc(case):
    lib = _lib.load()
    st = {s.name: s for s in SN.CASES}[case.p["case"]]
    n = len(st.sibs)
    flag = E._dt(st.dtype) | _lib.FUSE_ACC
    g = torch.Generator().manual_seed(5)
    I = [SN.inputs(st), _half(SN.inputs(dataclasses.replace(st, seed=st.seed + SEED2)))]
    for k, d in enumerate(I):     # the first sibling carries a bias, as in test_gpu_shared_fused_acc.py
        d["sibs"][0]["bias"] = ((torch.randn(st.sibs[0].d_out, generator=g) * 0.1) * (0.5 if k else 1.0)).to(st.dtype)
    b = GR.Bound(case.id)
    ar = b.arena(st.dtype)
    x = b.input(ar, (I[0]["x"], I[1]["x"]))
    dx = b.output(ar, "dx", (st.T, st.d_in), (I[0]["dx0"], I[1]["dx0"]))
    arr = (_lib.LayerArgs * n)()
    for i, sb in enumerate(st.sibs):
        q = [I[0]["sibs"][i], I[1]["sibs"][i]]
        v = {k: b.input(ar, _pair(q, k)) for k in ("A", "B", "Q", "R", "dy", "bias")}
        zeros = (lambda *s: (torch.zeros(*s), torch.zeros(*s))) if (st.grad_beta and i == 0) else (lambda *s: None)
        y, h = b.output(ar, f"y{i}", (st.T, sb.d_out)), b.output(ar, f"h{i}", (st.T, 64))
        dA, dB = b.output(ar, f"dA{i}", (st.d_in, sb.r), zeros(st.d_in, sb.r)), b.output(ar, f"dB{i}", (sb.r, sb.d_out), zeros(sb.r, sb.d_out))
        dbias = b.output(ar, f"dbias{i}", (sb.d_out,), zeros(sb.d_out)) if i == 0 else None
        ws = b.workspace(ar, lib.sow_workspace_bytes(st.T, st.d_in, sb.d_out, sb.r, sb.r_acc, _lib.ACC_LOWRANK, flag))
        arr[i] = _lib.LayerArgs(x=_p(x), A=_p(v["A"]), B=_p(v["B"]), acc_down=_p(v["Q"]), acc_up=_p(v["R"]), bias=_p(v["bias"]),
                                y=_p(y), h_save=_p(h), dy=_p(v["dy"]), dx=_p(dx), dA=_p(dA), dB=_p(dB), dbias=_p(dbias), T=st.T,
                                d_in=st.d_in, d_out=sb.d_out, r_live=sb.r, r_acc=sb.r_acc, acc_kind=_lib.ACC_LOWRANK, scale=sb.s,
                                grad_beta=st.grad_beta if i == 0 else 0.0, workspace=_p(ws), workspace_bytes=ws.numel())
    # the forward of such a set is the grouped one (sow_forward_shared refuses it); it must not write the shared dX
    fwd = (_lib.LayerArgs * n)(*[arr[i] for i in range(n)])
    for i in range(n):
        fwd[i].dx = None
        if i:
            arr[i].dx = None

    def call(rc):
        s = E._stream()
        rc(lib.sow_forward_group(fwd, n, flag, s), "sow_forward_group")
        rc(lib.sow_backward_shared(arr, n, flag, _lib.BWD_DATA | _lib.BWD_WEIGHTS, s), "sow_backward_shared")

    def check(k, out):
        d = I[k]
        for i, sb in enumerate(st.sibs):
            c = FA.case(f"{case.id}.s{i}", st.dtype, st.T, st.d_in, sb.d_out, sb.r, sb.r_acc, s=sb.s, bias=i == 0)
            FA.check(c, dict(d["sibs"][i], x=d["x"]), {key: out.get(f"{key}{i}") for key in ("y", "h", "dA", "dB", "dbias")})
        SN.check_dx(st, d, out["dx"])

    b.call, b.check = call, check
    return b


# ---------------------------------------------------------------------------------------------------------------- skinny forward
def build_skinny(case):
    lib = _lib.load()
    p = case.p
    dtype = DT[p["dtype"]]
    args = (dtype, p["T"], p["d_in"], p["d_out"], p["r"], p["bias"], p["acc"])

    def decided(d):
        """Whether every element of the hidden h = rn(s x A) is decided: test_gpu_skinny's reference rounds the exact
        projection, the kernel its fp32 sum, and the two can differ by one ulp of h only where the exact value lies within the
        fp32 accumulation noise of a rounding point.  A property of the inputs alone (float64), not of what the kernel gives."""
        xx, aa = to64(d["x"]), to64(d["A"])
        h, noise = p["s"] * (xx @ aa), fp32_floor(p["s"] ** 2 * ((xx * xx) @ (aa * aa)), p["d_in"])
        return bool((rne(h - noise, dtype) == rne(h + noise, dtype)).all())

    # the set that is checked against float64 (I2): the first seed whose hidden roundings are all decided
    second = next(d for d in (_half(SK._gauss(*args, seed=SEED2 + k)) for k in range(64)) if decided(d))
    I = [SK._gauss(*args, seed=0), second]
    kind = _lib.ACC_DENSE if p["acc"] == "dense" else _lib.ACC_NONE
    b = GR.Bound(case.id)
    ar = b.arena(dtype)
    x, A, B, bias, W = (b.input(ar, _pair(I, k)) for k in ("x", "A", "B", "bias", "W"))
    y = b.output(ar, "y", (p["T"], p["d_out"]))
    nws = lib.sow_forward_skinny_workspace_bytes(p["T"], p["d_in"], p["d_out"], p["r"], kind, E._dt(dtype))
    assert nws > 0
    ws = b.workspace(ar, nws)
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.acc_down, a.bias, a.y = (_p(t) for t in (x, A, B, W, bias, y))
    a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = p["T"], p["d_in"], p["d_out"], p["r"], kind, p["s"]
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    b.call = lambda rc: rc(lib.sow_forward_skinny(arr, 1, E._dt(dtype), E._stream()), "sow_forward_skinny")
    b.check = lambda k, out: SK._check(case.id, dtype, dict(I[k], s=p["s"]), out["y"])
    return b


# ---------------------------------------------------------------------------------------------------------------- sow_gemm_ex
def build_gemm(case):
    lib = _lib.load()
    p = case.p
    dtype = DT[p["dtype"]]
    dt = E._dt(dtype)
    M, N, K, beta = p["M"], p["N"], p["K"], p["beta"]

    def data(seed, scale):
        g = torch.Generator().manual_seed(M + N + K + seed)
        d = dict(a=torch.randn(M, K, generator=g), b=torch.randn(K, N, generator=g) * 0.05,
                 bias=torch.randn(N, generator=g) * 0.1 if p["bias"] else None, c0=torch.randn(M, N, generator=g) if beta else None)
        return {k: (None if v is None else (v * scale).to(dtype)) for k, v in d.items()}

    I = [data(0, 1.0), data(SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(dtype)
    A, B, Bi = (b.input(ar, _pair(I, k)) for k in ("a", "b", "bias"))
    C = b.output(ar, "C", (M, N), _pair(I, "c0"))
    nws = lib.sow_gemm_workspace_bytes(M, N, K, 0, dt) if p["use_ws"] else 0
    assert (nws > 0) == p["use_ws"], f"{case.id}: workspace query {nws}"
    ws = b.workspace(ar, nws)
    b.call = lambda rc: rc(lib.sow_gemm_ex(_p(A), K, 0, _p(B), N, 0, _p(C), N, _p(Bi), M, N, K, 1.0, beta, dt, _p(ws), nws,
                                           E._stream()), "sow_gemm_ex")

    def check(k, out):
        d = I[k]
        a64, b64 = to64(d["a"]), to64(d["b"])
        prod = a64 @ b64
        ref = prod + (to64(d["bias"]) if d["bias"] is not None else 0) + (beta * to64(d["c0"]) if beta else 0)
        sq = (a64 * a64) @ (b64 * b64)
        epi = gemm_epilogue(prod, 1.0, beta, d["c0"] if beta else None, d["bias"])
        if dtype == F32:
            check_bound(out["C"], ref, gemm_f32_bound(ref, sq, prod, K, epi), name=case.id)
        else:
            E._rounded(out["C"], ref, dtype, fp32_floor(sq, K) + epi, case.id)

    b.check = check
    return b


# ---------------------------------------------------------------------------------------------------------------- flat optimizer
def _opt_sets(n, pdtype, sdtype, step):
    a = SE._opt_data(n, pdtype, sdtype, step, seed=step)
    c = SE._opt_data(n, pdtype, sdtype, step, seed=step + SEED2)
    keys = ("p", "g", "m", "v")
    return [dict(zip(keys, a)), {k: (t * 0.5).to(t.dtype) for k, t in zip(keys, c)}]


def build_adamw_flat(case):
    lib = _lib.load()
    p = case.p
    pd, sd, n, step = DT[p["pdtype"]], DT[p["sdtype"]], p["n"], p["step"]
    hp = dict(lr=1e-3, betas=BETAS, eps=EPS, wd=0.1, step=step, grad_scale=0.5)
    I = _opt_sets(n, pd, sd, step)
    b = GR.Bound(case.id)
    arp, ars = b.arena(pd, 1), b.arena(sd, 1)          # one element off 16-byte alignment
    g = b.input(arp, _pair(I, "g"))
    pp = b.output(arp, "p", (n,), _pair(I, "p"))
    m, v = b.output(ars, "m", (n,), _pair(I, "m")), b.output(ars, "v", (n,), _pair(I, "v"))
    b.call = lambda rc: rc(lib.sow_adamw_flat(_p(pp), _p(g), _p(m), _p(v), n, hp["lr"], BETAS[0], BETAS[1], EPS, hp["wd"], step,
                                              hp["grad_scale"], SE.DT[pd], SE.DT[sd], E._stream()), "sow_adamw_flat")

    def check(k, out):
        d = I[k]
        refs, mags = adamw_ref(d["p"], d["g"], d["m"], d["v"], **hp)
        check_step(out, refs, mags, pd, sd, case.id)

    b.check = check
    return b


SEG_HP = ((1e-2, 0.1, 1), (3e-4, 0.0, 7), (1e-3, 0.05, 1000))      # lr, weight decay, step (test_gpu_adamw_segments.py)


def _seg_layout(lens):
    """segment 0 | segment 1 | a gap of 64 | segment 2 inside one guarded buffer."""
    b0, b1 = 0, lens[0]
    b2 = b1 + lens[1] + 64
    return [(b0, b1), (b1, b1 + lens[1]), (b2, b2 + lens[2])], b2 + lens[2]


def _seg_sets(total, ranges, pd, sd):
    I = _opt_sets(total, pd, sd, 7)
    for d in I:
        for (lo, hi), (_, _, step) in zip(ranges, SEG_HP):
            if step == 1:                                  # a first step starts from zero moments
                d["m"][lo:hi] = 0
                d["v"][lo:hi] = 0
    return I


def _check_segments(out, d, ranges, live, gm, pd, sd, name, steps=None):
    for key in ("p", "m", "v"):
        same = GR.bits(out[key]) == GR.bits(d[key])
        assert bool(same[~live].all()), f"{name}: {key} was rewritten outside every segment"
    for k, ((lo, hi), (lr, wd, step)) in enumerate(zip(ranges, SEG_HP)):
        refs, mags = adamw_ref(d["p"][lo:hi], d["g"][lo:hi], d["m"][lo:hi], d["v"][lo:hi], lr=lr, betas=BETAS, eps=EPS, wd=wd,
                               step=steps[k] if steps else step, grad_scale=gm)
        check_step({q: out[q][lo:hi] for q in ("p", "m", "v")}, refs, mags, pd, sd, f"{name} segment {k}")


def build_adamw_seg(case, stats=False):
    lib = _lib.load()
    p = case.p
    pd, sd = DT[p["pdtype"]], DT[p["sdtype"]]
    ranges, total = _seg_layout(p["lens"])
    I = _seg_sets(total, ranges, pd, sd)
    live = torch.zeros(total, dtype=torch.bool)
    for lo, hi in ranges:
        live[lo:hi] = True
    b = GR.Bound(case.id)
    arp, ars = b.arena(pd), b.arena(sd)
    g = b.input(arp, _pair(I, "g"))
    pp = b.output(arp, "p", (total,), _pair(I, "p"))
    m, v = b.output(ars, "m", (total,), _pair(I, "m")), b.output(ars, "v", (total,), _pair(I, "v"))
    rows = [(lo, hi, lr, wd, step) for (lo, hi), (lr, wd, step) in zip(ranges, SEG_HP)]
    segs = (_lib.AdamwSegment * len(rows))(*[_lib.AdamwSegment(*r) for r in rows])
    gs = 0.5
    if not stats:
        b.call = lambda rc: rc(lib.sow_adamw_flat_seg(_p(pp), _p(g), _p(m), _p(v), segs, len(rows), BETAS[0], BETAS[1], EPS, gs,
                                                      SE.DT[pd], SE.DT[sd], E._stream()), "sow_adamw_flat_seg")
        b.check = lambda k, out: _check_segments(out, I[k], ranges, live, gs, pd, sd, case.id)
        return b
    # the device record first (loss scale and skip counters on the device, clipping), then AdamW that reads it
    arf = b.arena(F32)
    ls_vals = (torch.tensor([4.0]), torch.tensor([2.0]))
    ls = b.input(arf, ls_vals)
    # skipped steps counted on the device: segment k reads counter cnt_idx[k] and corrects the bias for step - counter
    cnt_vals = (torch.tensor([0, 3, 0, 9], dtype=torch.int32), torch.tensor([1, 0, 2, 5], dtype=torch.int32))
    cnt_idx = (2, 0, 3)
    counters = b.extra("counters", torch.zeros(4, dtype=torch.int32, device=DEV), cnt_vals)
    idx = (ctypes.c_int * 3)(*cnt_idx)
    rec = b.workspace(arp, 32, key="record")
    ws = b.workspace(arp, lib.sow_grad_stats_workspace_bytes(total))
    max_norm = 1e-3

    def call(rc):
        s = E._stream()
        rc(lib.sow_grad_stats_flat(_p(g), total, SE.DT[pd], gs, max_norm, None, _p(ls), None, _p(counters), counters.numel(),
                                   _p(ws), ws.numel(), _p(rec), s), "sow_grad_stats_flat")
        rc(lib.sow_adamw_flat_seg_stats(_p(pp), _p(g), _p(m), _p(v), segs, idx, len(rows), BETAS[0], BETAS[1], EPS, _p(rec), 1,
                                        _p(counters), counters.numel(), SE.DT[pd], SE.DT[sd], s), "sow_adamw_flat_seg_stats")

    def check(k, out):
        d = I[k]
        r = dict(zip(("sumsq", "total_sq", "total_norm", "clip_coef", "grad_mult", "nonfinite"),
                     struct.unpack("<ddfffi", bytes(out["record"].numpy().tobytes()))))
        sq = R.sumsq(d["g"])
        ref = R.record(sq, grad_scale=float(torch.tensor(gs, dtype=F32)), loss_scale=float(ls_vals[k]),
                       max_norm=float(torch.tensor(max_norm, dtype=F32)))
        assert abs(r["sumsq"] - sq) <= R.sumsq_bound(total, sq), (r["sumsq"], sq)
        assert abs(r["total_sq"] - ref["total_sq"]) <= (total + 4) * 2.0 ** -52 * ref["total_sq"]
        for f in ("total_norm", "clip_coef", "grad_mult"):
            assert R.within_f32_ulps(r[f], ref[f]), (f, r[f], ref[f])
        assert r["nonfinite"] == 0 and ref["clip_coef"] < 1.0
        assert out["counters"].tolist() == cnt_vals[k].tolist(), "a finite step moved the skip counters"
        steps = [max(1, step - int(cnt_vals[k][ci])) for (_, _, step), ci in zip(SEG_HP, cnt_idx)]
        _check_segments(out, d, ranges, live, r["grad_mult"], pd, sd, case.id, steps=steps)

    b.call, b.check = call, check
    return b


def build_grad_stats(case):
    lib = _lib.load()
    p = case.p
    dtype, n = DT[p["dtype"]], p["n"]

    def data(seed, scale):
        g = torch.Generator().manual_seed(seed + n)
        return dict(g=(torch.randn(n, generator=g, dtype=torch.float64) * scale).to(dtype),
                    extra=torch.tensor([0.3 * n * scale * scale], dtype=torch.float64))

    I = [data(0, 1.0), data(SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar, ar64 = b.arena(dtype, 1), b.arena(torch.float64)
    g = b.input(ar, _pair(I, "g"))
    extra = b.input(ar64, _pair(I, "extra"))
    rec = b.workspace(ar, 32, key="record")
    ws = b.workspace(ar, lib.sow_grad_stats_workspace_bytes(n))
    gs, max_norm = 0.37, 7.0
    b.call = lambda rc: rc(lib.sow_grad_stats_flat(_p(g), n, SE.DT[dtype], gs, max_norm, _p(extra), None, None, None, 0, _p(ws),
                                                   ws.numel(), _p(rec), E._stream()), "sow_grad_stats_flat")

    def check(k, out):
        d = I[k]
        r = dict(zip(("sumsq", "total_sq", "total_norm", "clip_coef", "grad_mult", "nonfinite"),
                     struct.unpack("<ddfffi", bytes(out["record"].numpy().tobytes()))))
        sq = R.sumsq(d["g"])
        ref = R.record(sq, grad_scale=float(torch.tensor(gs, dtype=F32)), max_norm=max_norm, extra_sq=float(d["extra"]))
        assert abs(r["sumsq"] - sq) <= R.sumsq_bound(n, sq), (r["sumsq"], sq)
        assert abs(r["total_sq"] - ref["total_sq"]) <= (n + 4) * 2.0 ** -52 * ref["total_sq"]
        for f in ("total_norm", "clip_coef", "grad_mult"):
            assert R.within_f32_ulps(r[f], ref[f]), (f, r[f], ref[f])
        assert r["nonfinite"] == 0 and ref["clip_coef"] < 1.0

    b.check = check
    return b


def build_zero(case):
    """sow_zero_state (ops.zero_) over byte spans of 1 .. 17 bytes at misaligned starts and a few long ones, more buffers than
    one launch takes (test_gpu_step_elementwise.test_zero_state_spans)."""
    lib = _lib.load()
    nsp = case.p["spans"]
    spans, pos = [], 0
    for i in range(nsp):
        n = 1 + i % 17 if i < 51 else [1001, 4096, 70001, 3, 16, 17, 31, 65, 100003][i - 51]
        start = pos + 1 + (i % 15)
        spans.append((start, n))
        pos = start + n + 16
    size = pos + 64
    gen = torch.Generator().manual_seed(3)
    fills = tuple(torch.randint(1, 256, (size,), generator=gen, dtype=torch.int32).to(torch.uint8) for _ in range(2))
    b = GR.Bound(case.id)
    pool = b.extra("pool", torch.zeros(size, dtype=torch.uint8, device=DEV), fills)
    ptrs = (ctypes.c_void_p * nsp)(*[pool.data_ptr() + s for s, _ in spans])
    sizes = (ctypes.c_int64 * nsp)(*[n for _, n in spans])
    b.call = lambda rc: rc(lib.sow_zero_state(ptrs, sizes, nsp, E._stream()), "sow_zero_state")

    def check(k, out):
        mask = torch.zeros(size, dtype=torch.bool)
        for s, n in spans:
            mask[s:s + n] = True
        assert bool((out["pool"][mask] == 0).all()), "a byte of a zeroed span is not 0"
        assert torch.equal(out["pool"][~mask], fills[k][~mask]), "a byte outside the spans was written"

    b.check = check
    return b


# ---------------------------------------------------------------------------------------------------------------- tensor trains
def build_tt_reconstruct(case):
    lib = _lib.load()
    specs = [TTE.S[k] for k in case.p["specs"]]
    n = len(specs)

    def data(seed, scale):
        gen = torch.Generator().manual_seed(seed)
        return [[torch.randn(sh, generator=gen) * (scale if k == 0 else 1.0) for k, sh in enumerate(T.core_shapes(s[2], s[3], s[4]))]
                for s in specs]

    I = [data(1, 1.0), data(1 + SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    descs, outs, lds = [], [], []
    for i, s in enumerate(specs):
        cores = [b.input(ar, (I[0][i][k], I[1][i][k])) for k in range(len(s[3]))]
        o = b.output(ar, f"m{i}", (s[0], s[1]))
        descs.append(TTE._desc(cores, s)), outs.append(o.data_ptr()), lds.append(s[1])
    arr = (_lib.TtDesc * n)(*descs)
    a_out, a_ld = (ctypes.c_void_p * n)(*outs), (ctypes.c_int64 * n)(*lds)
    b.call = lambda rc: rc(lib.sow_tt_reconstruct_batch(arr, a_out, a_ld, n, E._stream()), "sow_tt_reconstruct_batch")

    def check(k, out):
        for i, s in enumerate(specs):
            T.check_tt_matrix(out[f"m{i}"], I[k][i], s[3], s[4], s[0], s[1], name=f"{case.id}[{i}]")

    b.check = check
    return b


def build_tt_decompose(case):
    lib = _lib.load()
    specs = [TTE.S[k] for k in case.p["specs"]]
    n = len(specs)

    def data(seed, scale):
        gen = torch.Generator().manual_seed(seed)
        return [TTE._gauss(s[0], s[1], gen) * (0.5 + i % 3) * scale for i, s in enumerate(specs)]

    I = [data(2, 1.0), data(2 + SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    descs, srcs, lds, wsp, wsb = [], [], [], [], []
    for i, s in enumerate(specs):
        cores = [b.output(ar, f"c{i}.{k}", sh) for k, sh in enumerate(T.core_shapes(s[2], s[3], s[4]))]
        d = TTE._desc(cores, s)
        src = b.input(ar, (I[0][i], I[1][i]))
        nb = int(lib.sow_tt_decompose_workspace_bytes(ctypes.byref(d)))
        assert nb > 0
        ws = b.workspace(ar, nb)
        descs.append(d), srcs.append(src.data_ptr()), lds.append(s[1]), wsp.append(ws.data_ptr()), wsb.append(nb)
    arr = (_lib.TtDesc * n)(*descs)
    a_src, a_ld = (ctypes.c_void_p * n)(*srcs), (ctypes.c_int64 * n)(*lds)
    a_ws, a_wb = (ctypes.c_void_p * n)(*wsp), (ctypes.c_size_t * n)(*wsb)
    b.call = lambda rc: rc(lib.sow_tt_decompose_batch(arr, a_src, a_ld, n, a_ws, a_wb, E._stream()), "sow_tt_decompose_batch")

    def check(k, out):
        for i, s in enumerate(specs):
            rows, cols, ranks, ind, outd = s
            cores = [out[f"c{i}.{q}"] for q in range(len(ind))]
            T.check_tt_decomposition(cores, T.pad_interleave_ref(I[k][i], ind, outd), ranks, ind, outd, name=f"{case.id}[{i}]")

    b.check = check
    return b


def build_ttadam_batch(case):
    lib = _lib.load()
    items = [(TTE.S[k], has) for k, has in case.p["items"]]
    n = len(items)
    lr_wd = 1e-5

    def data(seed, scale):
        gen = torch.Generator().manual_seed(seed)
        out = []
        for s, has in items:
            inp = TTE.adam_item_inputs(s, has, BETAS, lr_wd, gen)
            if scale != 1.0:       # p, g and m halved, v quartered: the update m / sqrt(v) keeps its size
                inp["p0"], inp["g"] = inp["p0"] * scale, inp["g"] * scale
                if has:
                    inp["cores_m0"] = [c * (scale if k == 0 else 1.0) for k, c in enumerate(inp["cores_m0"])]
                    inp["cores_v0"] = [c * (scale * scale if k == 0 else 1.0) for k, c in enumerate(inp["cores_v0"])]
            out.append(inp)
        return out

    I = [data(1000, 1.0), data(1000 + SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    its = []
    for i, (s, has) in enumerate(items):
        rows, cols = s[0], s[1]
        shapes = T.core_shapes(s[2], s[3], s[4])
        init = lambda key, k, sh: (I[0][i][key][k].reshape(sh), I[1][i][key][k].reshape(sh)) if has else None   # noqa: E731
        cm = [b.output(ar, f"m{i}.{k}", sh, init("cores_m0", k, sh)) for k, sh in enumerate(shapes)]
        cv = [b.output(ar, f"v{i}.{k}", sh, init("cores_v0", k, sh)) for k, sh in enumerate(shapes)]
        pp = b.output(ar, f"p{i}", (rows, cols), (I[0][i]["p0"], I[1][i]["p0"]))
        g = b.input(ar, (I[0][i]["g"], I[1][i]["g"]))
        it = _lib.TtAdamItem()
        it.m, it.v = TTE._desc(cm, s), TTE._desc(cv, s)
        nb = int(lib.sow_ttadam_workspace_bytes(ctypes.byref(it.m)))
        ws = b.workspace(ar, nb)
        it.param, it.grad, it.ld_param, it.ld_grad = pp.data_ptr(), g.data_ptr(), cols, cols
        it.step_size, it.lr_times_wd, it.has_state = I[0][i]["step_size"], I[0][i]["lr_wd"], has
        it.workspace, it.workspace_bytes = ws.data_ptr(), nb
        its.append(it)
    arr = (_lib.TtAdamItem * n)(*its)
    b.call = lambda rc: rc(lib.sow_ttadam_batch(arr, n, BETAS[0], BETAS[1], 1e-8, E._stream()), "sow_ttadam_batch")

    def check(k, out):
        undecided = 0
        for i, (s, has) in enumerate(items):
            d = len(s[3])
            st = T.check_ttadam_batch(out[f"p{i}"], [out[f"m{i}.{q}"] for q in range(d)], [out[f"v{i}.{q}"] for q in range(d)],
                                      I[k][i], name=f"{case.id}[{i} state={has}]", max_undecided=None)
            undecided += st["p"]["undecided_count"]
        TTE._assert_decided(case.id, undecided, sum(inp["p0"].numel() for inp in I[k]))

    b.check = check
    return b


def build_ttadam_dense(case):
    lib = _lib.load()
    n = case.p["n"]
    I = _opt_sets(n, F32, F32, 3)
    for d in I:
        d["v"][::7] = -d["v"][::7]                          # negative moments of a lossy TT re-compression (clamped)
    lr, step, wd = 1e-2, 3, 0.01
    step_size = float(torch.tensor(lr * math.sqrt(1 - BETAS[1] ** step) / (1 - BETAS[0] ** step)).float())
    lr_wd = float(torch.tensor(lr * wd).float())
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    g = b.input(ar, _pair(I, "g"))
    pp, m, v = (b.output(ar, k, (n,), _pair(I, k)) for k in ("p", "m", "v"))
    b.call = lambda rc: rc(lib.sow_ttadam_dense(_p(pp), _p(g), _p(m), _p(v), n, BETAS[0], BETAS[1], 1e-8, step_size, lr_wd, 1,
                                                E._stream()), "sow_ttadam_dense")

    def check(k, out):
        d = I[k]
        refs, mags = ttadam_ref(d["p"], d["g"], d["m"], d["v"], betas=BETAS, eps=1e-8, step_size=step_size, lr_wd=lr_wd, clamp_v=True)
        check_step(out, refs, mags, F32, F32, case.id)

    b.check = check
    return b


def build_kron(case):
    lib = _lib.load()
    p = case.p
    ra0, rb0, ij, ra1, rb1 = (p[k] for k in ("ra0", "rb0", "ij", "ra1", "rb1"))

    def data(seed, scale):
        g = torch.Generator().manual_seed(seed)
        return dict(A=torch.randn(ra0, ij, ra1, generator=g) * scale, B=torch.randn(rb0, ij, rb1, generator=g))

    I = [data(6, 1.0), data(6 + SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    A, B = b.input(ar, _pair(I, "A")), b.input(ar, _pair(I, "B"))
    out = b.output(ar, "o", (ra0 * rb0, ij, ra1 * rb1))
    b.call = lambda rc: rc(lib.sow_tt_kron_core(_p(A), _p(B), _p(out), ra0, rb0, ij, ra1, rb1, E._stream()), "sow_tt_kron_core")

    def check(k, res):      # an fp32 product is correctly rounded on both sides: bit-exact against the CPU
        ref = torch.einsum("aeb,ced->acebd", I[k]["A"].double(), I[k]["B"].double()).reshape(ra0 * rb0, ij, ra1 * rb1).float()
        assert torch.equal(GR.bits(res["o"]), GR.bits(ref))

    b.check = check
    return b


def build_inverse(case):
    lib = _lib.load()
    batch, r = case.p["batch"], case.p["r"]
    g = torch.Generator().manual_seed(10)
    I = [dict(A=torch.randn(batch, r, r, generator=g)), dict(A=torch.randn(batch, r, r, generator=g) * 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    A = b.input(ar, _pair(I, "A"))
    X = b.output(ar, "X", (batch, r, r))
    b.call = lambda rc: rc(lib.sow_small_inverse(_p(A), _p(X), batch, r, E._stream()), "sow_small_inverse")

    def check(k, out):      # test_gpu_step_elementwise.test_small_inverse_residual
        A64, X64 = I[k]["A"].double(), out["X"].double()
        P, L, U = torch.linalg.lu(A64)
        err = A64 @ X64 - torch.eye(r, dtype=torch.float64)
        check_bound(err, torch.zeros_like(err), 8 * r * U32 * (P @ (L.abs() @ U.abs())) @ X64.abs(), name=f"{case.id}: A X - I")

    b.check = check
    return b


def build_absmax(case):
    lib = _lib.load()
    n = case.p["n"]
    g = torch.Generator().manual_seed(8)
    I = [dict(x=torch.randn(n, generator=g) * 3), dict(x=torch.randn(n, generator=g) * 1.5)]
    b = GR.Bound(case.id)
    ar = b.arena(F32)
    x = b.input(ar, _pair(I, "x"))
    o = b.output(ar, "o", (1,))
    b.call = lambda rc: rc(lib.sow_absmax(_p(x), n, _p(o), E._stream()), "sow_absmax")

    def check(k, out):
        assert float(out["o"]) == float(I[k]["x"].abs().max())

    b.check = check
    return b


def build_axpby(case):
    lib = _lib.load()
    dtype, n = DT[case.p["dtype"]], case.p["n"]
    a, bb = 0.7, -1.3

    def data(seed, scale):
        g = torch.Generator().manual_seed(seed)
        return dict(x=(torch.randn(n, generator=g) * scale).to(dtype), y=(torch.randn(n, generator=g) * scale).to(dtype))

    I = [data(4, 1.0), data(4 + SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(dtype)
    x = b.input(ar, _pair(I, "x"))
    y = b.output(ar, "y", (n,), _pair(I, "y"))
    b.call = lambda rc: rc(lib.sow_axpby(_p(x), _p(y), n, a, bb, SE.DT[dtype], E._stream()), "sow_axpby")

    def check(k, out):      # test_gpu_step_elementwise.test_axpby_single_rounding
        af, bf = float(torch.tensor(a).float()), float(torch.tensor(bb).float())
        x0, y0 = to64(I[k]["x"]), to64(I[k]["y"])
        ref = af * x0 + bf * y0
        noise = 2 * U32 * (abs(af) * x0.abs() + abs(bf) * y0.abs())
        if dtype == F32:
            check_bound(out["y"], ref, ulp(ref, F32) + noise, name=case.id)
        else:
            check_rounded_noisy(out["y"], ref, dtype, noise + ulp(ref, F32), name=case.id)

    b.check = check
    return b


def build_cast(case):
    lib = _lib.load()
    p = case.p
    src, dst = DT[p["src"]], DT[p["dst"]]
    b = GR.Bound(case.id)
    ars, ard = b.arena(src), (b.arena(dst))
    if p["strided"]:
        rows, cols = p["rows"], p["cols"]
        g = torch.Generator().manual_seed(3)
        I = [dict(x=torch.randn(rows, cols + 3, generator=g).to(src)), dict(x=(torch.randn(rows, cols + 3, generator=g) * 0.5).to(src))]
        x = b.input(ars, _pair(I, "x"))
        y = b.output(ard, None, (rows, cols + 2))
        b.outs["y"] = y[:, :cols]          # the two padding elements of every row are not the kernel's to write
        b.call = lambda rc: rc(lib.sow_cast_copy(_p(x), cols + 3, SE.DT[src], _p(y), cols + 2, SE.DT[dst], rows, cols, E._stream()),
                               "sow_cast_copy")

        def check(k, out):      # the fill before replay 2 was 0x00: the padding of every row still holds zero bits
            assert torch.equal(GR.bits(out["y"].contiguous()), GR.bits(I[k]["x"][:, :cols].to(dst).contiguous()))
            assert bool((GR.bits(y[:, cols:].contiguous()) == 0).all()), "the row padding of a strided output was written"
    else:
        n = p["n"]
        vals = SE._cast_sources()[src]
        reps = -(-n // vals.numel())
        base = vals.repeat(reps)[:n]
        I = [dict(x=base), dict(x=base.flip(0))]
        x = b.input(ars, _pair(I, "x"))
        y = b.output(ard, "y", (n,))
        b.call = lambda rc: rc(lib.sow_cast_copy(_p(x), n, SE.DT[src], _p(y), n, SE.DT[dst], 1, n, E._stream()), "sow_cast_copy")

        def check(k, out):      # bit-exact against torch's cast, NaN for NaN
            ref = I[k]["x"].to(dst)
            ok = (GR.bits(out["y"]) == GR.bits(ref)) | (torch.isnan(out["y"].float()) & torch.isnan(ref.float()))
            assert bool(ok.all()), f"{case.id}: {int((~ok).sum())} elements differ from torch's cast"
    b.check = check
    return b


# ---------------------------------------------------------------------------------------------------------------- QR, accumulate
def build_qr(case):
    lib = _lib.load()
    p = case.p
    m, n, k, din, dout, need_r, extra = p["m"], p["n"], p["k"], DT[p["din"]], DT[p["dout"]], p["need_r"], p["extra_ld"]

    def data(seed, scale):
        W = (torch.randn(m, n, generator=torch.Generator().manual_seed(m + n + k + seed)) * scale).to(din)
        return dict(W=W, Wp=torch.cat([W, torch.zeros(m, extra, dtype=din)], 1) if extra else W)

    I = [data(0, 1.0), data(SEED2, 0.5)]
    b = GR.Bound(case.id)
    ari, aro = b.arena(din), b.arena(dout)
    W = b.input(ari, _pair(I, "Wp"))
    Q = b.output(aro, "Q", (m, k))
    Rm = b.output(aro, "R", (k, n)) if need_r else None
    ws = b.workspace(aro, lib.sow_qr_workspace_bytes(m, n, k, SE.DT[din], need_r))
    b.call = lambda rc: rc(lib.sow_qr_thin(_p(W), n + extra, m, n, SE.DT[din], k, _p(Q), k, _p(Rm), n, SE.DT[dout], _p(ws),
                                           ws.numel(), E._stream()), "sow_qr_thin")
    b.check = lambda j, out: check_qr(I[j]["W"], out["Q"], out.get("R"), k, dout, name=case.id)
    return b


def build_accumulate(case):
    """sow_accumulate_batch on a few items of test_gpu_step_elementwise._acc_items: rank update of the dense accumulator
    (beta 0 and 1), the QR of the draw into A_new (aliasing A or not), the zeroed byte spans."""
    lib = _lib.load()
    dtype = DT[case.p["dtype"]]
    items = SE._acc_items(dtype)[:case.p["items"]]
    nit = len(items)

    def data(seed, scale):
        g = torch.Generator().manual_seed(seed)
        out = []
        for it in items:
            d_in, d_out, r = it["d_in"], it["d_out"], it["r"]
            d = dict(A=(torch.randn(d_in, r, generator=g) * 0.05 * scale).to(dtype), B=(torch.randn(r, d_out, generator=g) * 0.05).to(dtype),
                     acc=(torch.randn(d_in, d_out, generator=g) * 0.01 * scale).to(dtype))
            if it["draw"]:
                cols = {"r": r, "more": r + 5, "d_out": d_out}[it["draw"]]
                d["D"] = (torch.randn(d_in, cols + 3, generator=g) * scale).to(dtype)
            out.append(d)
        return out

    I = [data(5, 1.0), data(5 + SEED2, 0.5)]
    b = GR.Bound(case.id)
    ar = b.arena(dtype)
    args = (_lib.AccumulateArgs * nit)()
    gen = torch.Generator().manual_seed(7)
    fills = tuple(torch.randint(1, 256, (nit * 64,), generator=gen, dtype=torch.int32).to(torch.uint8) for _ in range(2))
    zpool = b.extra("zpool", torch.zeros(nit * 64, dtype=torch.uint8, device=DEV), fills)
    zspans = []
    for i, it in enumerate(items):
        d_in, d_out, r = it["d_in"], it["d_out"], it["r"]
        q = [I[0][i], I[1][i]]
        acc = b.output(ar, f"acc{i}", (d_in, d_out), _pair(q, "acc") if it["beta"] else None)   # beta = 0: poisoned, never read
        Bd = b.input(ar, _pair(q, "B"))
        a = args[i]
        if it["draw"]:
            cols = {"r": r, "more": r + 5, "d_out": d_out}[it["draw"]]
            Dd = b.input(ar, _pair(q, "D"))
            ws = b.workspace(ar, lib.sow_qr_workspace_bytes(d_in, cols, r, SE.DT[dtype], 0) + 256)
            a.draw, a.ld_draw, a.draw_cols = _p(Dd), cols + 3, cols
            a.workspace, a.workspace_bytes = _p(ws), ws.numel()
        if it["draw"] and it["alias"]:
            A = b.output(ar, f"Anew{i}", (d_in, r), _pair(q, "A"))        # A_new = A: overwritten after the update read it
            a.A_new = _p(A)
        else:
            A = b.input(ar, _pair(q, "A"))
            if it["draw"]:
                a.A_new = _p(b.output(ar, f"Anew{i}", (d_in, r)))
        a.acc, a.A, a.B = _p(acc), _p(A), _p(Bd)
        a.d_in, a.d_out, a.r, a.r_new = d_in, d_out, r, r
        a.scale, a.acc_beta = it["scale"], it["beta"]
        zoff, zlen = i * 64 + it["zero"][0], it["zero"][1]
        a.zero, a.zero_bytes = zpool.data_ptr() + zoff, zlen
        zspans.append((zoff, zlen))
    b.call = lambda rc: rc(lib.sow_accumulate_batch(args, nit, SE.DT[dtype], E._stream()), "sow_accumulate_batch")

    def check(k, out):
        mask = torch.zeros(nit * 64, dtype=torch.bool)
        for i, it in enumerate(items):
            d = I[k][i]
            mask[zspans[i][0]:zspans[i][0] + zspans[i][1]] = True
            check_rank_update(out[f"acc{i}"], d["acc"], d["A"], d["B"], it["scale"], it["beta"], dtype, name=f"{case.id} item {i} acc")
            if it["draw"]:
                check_qr(d["D"][:, :it["r"]], out[f"Anew{i}"], None, it["r"], dtype, name=f"{case.id} item {i} A_new")
        assert bool((out["zpool"][mask] == 0).all()), "zero: a byte of a zeroed span is not 0"
        assert torch.equal(out["zpool"][~mask], fills[k][~mask]), "zero: a byte outside the zeroed spans was written"

    b.check = check
    return b


BUILDERS = dict(layer=build_layer, group=build_group, shared=build_shared, shared_acc=build_shared_acc, skinny=build_skinny,
                gemm=build_gemm, adamw_flat=build_adamw_flat, adamw_seg=build_adamw_seg,
                adamw_seg_stats=lambda c: build_adamw_seg(c, stats=True), grad_stats=build_grad_stats, zero=build_zero,
                tt_reconstruct=build_tt_reconstruct, tt_decompose=build_tt_decompose, ttadam_batch=build_ttadam_batch,
                ttadam_dense=build_ttadam_dense, kron=build_kron, inverse=build_inverse, absmax=build_absmax, axpby=build_axpby,
                cast=build_cast, qr=build_qr, accumulate=build_accumulate)


def _switches(case):
    if case.kind == "layer":
        return dict(case.p["layer"].switches)
    return dict(case.p.get("switches", {}))


@pytest.mark.parametrize("case", GP.CASES, ids=lambda c: c.id)
def test_replay(case):
    trace = TRACES[case.id] = []
    with _lib.switch(**_switches(case)):       # the workspace plans and the dispatch both read the switches
        b = BUILDERS[case.kind](case)
        GR.replay(b, trace)
    missing = [k for k in case.claims if not GR.has_kernel(trace, k)]
    assert not missing, f"{case.id}: claims {missing}, the eager trace holds {sorted(set(trace))}"


# ---------------------------------------------------------------------------------------------------------------- training step
T_STEP, D_STEP, FF_STEP, R_STEP = 8193, 64, 128, 16
FINITE_SCALE, OVERFLOW_SCALE = 8.0, 3.0e38      # x dY: the second one overflows f32, bf16 and f16


class _Mlp(nn.Module):
    """Two siblings on one input and one following layer, under the names group_siblings looks for."""

    def __init__(self, dtype, seed=11):
        super().__init__()
        from sow_amd import SoWLinear
        g = torch.Generator().manual_seed(seed)
        self.mlp = nn.Module()

        def mk(i, o):
            m = SoWLinear(i, o, bias=False, rank=R_STEP, init_method="normal", scale=0.5, device=DEV, dtype=dtype)
            with torch.no_grad():
                m.downscale_weights[0].copy_((torch.randn(i, R_STEP, generator=g) / i ** 0.5).to(dtype))
                m.upscale_weights[0].copy_((torch.randn(R_STEP, o, generator=g) * 0.1).to(dtype))
            return m

        self.mlp.gate_proj, self.mlp.up_proj, self.mlp.down_proj = mk(D_STEP, FF_STEP), mk(D_STEP, FF_STEP), mk(FF_STEP, D_STEP)

    def forward(self, x):
        m = self.mlp
        return m.down_proj(m.gate_proj(x) * m.up_proj(x))


def _record(buf):
    return dict(zip(("sumsq", "total_sq", "total_norm", "clip_coef", "grad_mult", "nonfinite"),
                    struct.unpack("<ddfffi", bytes(buf.cpu().numpy().tobytes()))))


@pytest.mark.parametrize("dtype,groups", [(BF16, False), (F16, True)], ids=["bf16", "f16_two_groups"])
def test_step_forward_backward_optimizer_in_one_graph(dtype, groups):
    """forward + backward + FactorAdamW.step(loss_scale=<device tensor>, max_grad_norm=1, skip_nonfinite=True) +
    bucket.zero_grad() captured once on a side stream and replayed on a finite batch, an overflowing one and a finite one,
    the batch changed in place; the eager twin runs the same events from the same state.  A replay repeats the captured
    host step number, so the twin resets its host step counts to the captured value before each step."""
    from sow_amd import FactorAdamW, FactorBucket, factor_parameters, group_siblings
    net = _Mlp(dtype)
    assert group_siblings(net, shared_input=True) == 1
    bucket = FactorBucket(factor_parameters(net))
    assert bucket.attach(net) == 3
    ps = bucket.params
    pg = [{"params": ps[:2] + ps[3:5], "lr": 1e-2, "weight_decay": 0.1},
          {"params": [ps[2], ps[5]], "lr": 3e-3, "weight_decay": 0.0}] if groups else None
    opt = FactorAdamW(bucket, lr=5e-3, weight_decay=0.05, state_dtype=F32, param_groups=pg)
    x = torch.empty(T_STEP, D_STEP, dtype=dtype, device=DEV)
    w = torch.empty(T_STEP, D_STEP, dtype=F32, device=DEV)
    scale_t = torch.empty(1, dtype=F32, device=DEV)
    g_keep = torch.zeros_like(bucket.flat_grad)        # the gradient of the step, kept before zero_grad() clears it
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True)

    def batch(seed, scale):
        g = torch.Generator().manual_seed(seed)
        x.copy_(torch.randn(T_STEP, D_STEP, generator=g).to(dtype))
        w.copy_(torch.randn(T_STEP, D_STEP, generator=g))
        scale_t.fill_(scale)

    def step():
        y = net(x)
        y.backward((w * scale_t).to(dtype))
        st = opt.step(loss_scale=scale_t, **kw)
        g_keep.copy_(bucket.flat_grad)
        bucket.zero_grad()
        return st

    # one eager step first: it creates the counters, the record, the sinks' workspaces and the reduction descriptors
    bucket.zero_grad()
    batch(1, FINITE_SCALE)
    st0 = step()
    torch.cuda.synchronize()
    assert _record(st0.buf)["nonfinite"] == 0
    state = (bucket.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.skip_counters)
    s0 = [t.clone() for t in state]
    host0 = (opt.step_count, list(opt.group_steps) if groups else None)

    def restore_host():
        opt.step_count = host0[0]
        if groups:
            opt.group_steps = list(host0[1])

    def restore():
        for dst, src in zip(state, s0):
            dst.copy_(src)
        restore_host()

    def snapshot(st):
        torch.cuda.synchronize()
        return [GR.bits(t).clone() for t in state] + [st.buf.clone(), GR.bits(g_keep).clone()]

    events = [(2, FINITE_SCALE), (3, OVERFLOW_SCALE), (4, FINITE_SCALE)]
    # the eager twin: the three events in sequence from the saved state
    eager = []
    for seed, scale in events:
        batch(seed, scale)
        restore_host()
        eager.append(snapshot(step()))
    # capture on a side stream, from the saved state
    restore()
    batch(2, FINITE_SCALE)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # warm-up on the capturing stream
    side.synchronize()
    restore()
    torch.cuda.synchronize()
    before = [t.clone() for t in state]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st_graph = step()
    torch.cuda.synchronize()
    for t, b0 in zip(state, before):
        assert torch.equal(GR.bits(t), GR.bits(b0)), "capturing the step ran something"
    names = ("flat_param", "exp_avg", "exp_avg_sq", "skip counters", "record", "gradient")
    prev = [GR.bits(t).clone() for t in s0]
    for k, (seed, scale) in enumerate(events):
        batch(seed, scale)
        graph.replay()
        got = snapshot(st_graph)
        for nm, a, e in zip(names, got, eager[k]):
            assert torch.equal(a, e), f"event {k}: {nm} of the replay differs from the eager twin"
        rec = _record(got[4])
        if scale == OVERFLOW_SCALE:
            assert rec["nonfinite"] == 1
            for nm, a, e in zip(names[:3], got[:3], prev[:3]):
                assert torch.equal(a, e), f"the overflowing event moved {nm}"
            assert got[3].cpu().tolist() == (prev[3] + 1).cpu().tolist(), "the skip counters did not advance by one"
        else:
            assert rec["nonfinite"] == 0 and not torch.equal(got[0], prev[0])
            assert got[3].cpu().tolist() == prev[3].cpu().tolist()
        if k < len(events) - 1:
            prev = got
    # the last event against float64 AdamW (tests/step_numerics.py, as test_gpu_step_elementwise.py holds sow_adamw_flat): the
    # gradient the step saw, the record's own multiplier, the bias correction of host step - skipped steps
    p0, m0, v0 = (t.view(dt).cpu() for t, dt in zip(prev[:3], (dtype, F32, F32)))
    cnt = prev[3].cpu().tolist()
    grad = got[5].view(dtype).cpu()
    out = dict(p=bucket.flat_param.cpu(), m=opt.exp_avg.cpu(), v=opt.exp_avg_sq.cpu())
    if groups:
        table = [(b_, e_, opt._groups[gi]["lr"], opt._groups[gi]["weight_decay"], host0[1][gi] + 1 - cnt[gi])
                 for gi, b_, e_ in opt._group_ranges()]
    else:
        table = [(0, bucket.padded_numel, opt.lr, opt.weight_decay, host0[0] + 1 - cnt[0])]
    assert all(step_eff == host0[0] for *_, step_eff in table)           # one skipped step taken off the captured number
    for lo, hi, lr, wd, step_eff in table:
        refs, mags = adamw_ref(p0[lo:hi], grad[lo:hi], m0[lo:hi], v0[lo:hi], lr=lr, betas=opt.betas, eps=opt.eps, wd=wd,
                               step=step_eff, grad_scale=rec["grad_mult"])
        check_step({q: t[lo:hi] for q, t in out.items()}, refs, mags, dtype, F32, f"step [{lo}, {hi})")
    ref = R.record(R.sumsq(grad), loss_scale=FINITE_SCALE, max_norm=1.0)
    assert R.within_f32_ulps(rec["grad_mult"], ref["grad_mult"]) and ref["clip_coef"] < 1.0


def test_step_cached_groups_follow_factors_updated_in_place():
    """ops.LayerGroup / ops.SharedInputGroup / ops.DeferredReduce over static buffers, their argument arrays and reduction
    descriptors built once: forward, shared data gradient, deferred weight gradients and one reduction captured in one graph
    and replayed after A and B were updated in place (what the optimizer does between replays) -- the cached pointers and
    every pack follow the data: bit-identical to the eager calls on the updated factors, and within the float64 bounds."""
    from sow_amd import ops
    dtype = BF16
    st = SI.Set("cached_groups", dtype, T_STEP, D_STEP, [SI.Sib(FF_STEP, R_STEP, False, 0.5), SI.Sib(D_STEP, 8, True, 1.0)])
    dev = lambda t: None if t is None else t.to(DEV, dtype)   # noqa: E731
    x0, per0, _ = SI._data(st, seed=0)
    x = dev(x0)
    per = [{k: dev(v) for k, v in q.items()} for q in per0]
    dxs = torch.empty(T_STEP, D_STEP, dtype=dtype, device=DEV)
    outs = [(torch.zeros_like(q["A"]), torch.zeros_like(q["B"]), None if q["bias"] is None else torch.zeros_like(q["bias"])) for q in per]
    fwd = ops.LayerGroup([ops.LayerCall(x, q["A"], q["B"], bias=q["bias"], scale=sb.s) for q, sb in zip(per, st.sibs)])
    hs, ys = [c.h for c in fwd.calls], [c.y for c in fwd.calls]
    calls = [ops.LayerCall(x, q["A"], q["B"], bias=q["bias"], scale=sb.s, h=h, y=y, dy2=q["dy"], dx=dxs, out=o, grad_beta=0.0)
             for q, sb, h, y, o in zip(per, st.sibs, hs, ys, outs)]
    bwd = ops.SharedInputGroup(calls)
    red = ops.DeferredReduce()
    phases = _lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS

    def step():
        fwd.forward()
        assert bwd.backward(phases), "the shared-input kernels did not admit the set"
        red.add_group(bwd, phases)
        red.run()

    def snapshot():
        torch.cuda.synchronize()
        return [GR.bits(t).clone() for t in ys + hs + [dxs] + [g for o in outs for g in o if g is not None]]

    def factors(seed, scale):
        _, q2, _ = SI._data(st, seed=seed)
        for q, n in zip(per, q2):
            for k in ("A", "B", "bias"):
                if q[k] is not None:
                    q[k].copy_((n[k] * scale).to(dtype))

    step()                                              # first use: the descriptors of the deferred reduction go to the device
    eager = []
    for seed, scale in ((0, 1.0), (SEED2, 0.5)):
        factors(seed, scale)
        step()
        eager.append(snapshot())
    assert not torch.equal(eager[0][0], eager[1][0])
    factors(0, 1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    for k, (seed, scale) in enumerate(((0, 1.0), (SEED2, 0.5), (SEED2, 0.5))):
        factors(seed, scale)
        if k < 2:                                       # the third replay runs on what the second left everywhere
            for t in ys + hs + [dxs]:
                GR.bits(t).fill_(-1 if k == 0 else 0)
        torch.cuda.synchronize()
        graph.replay()
        got = snapshot()
        for i, (a, e) in enumerate(zip(got, eager[min(k, 1)])):
            assert torch.equal(a, e), f"replay {k}: tensor {i} differs from the eager calls on the same factors"
    # the outputs of the last replay against float64 (the checks of test_gpu_elementwise.py and test_gpu_shared_input.py)
    cpu = [{k: (None if v is None else v.cpu()) for k, v in q.items()} for q in per]
    for i, (sb, q) in enumerate(zip(st.sibs, cpu)):
        c = E.Case(f"cached_groups.s{i}", dtype, st.T, st.d_in, sb.d_out, sb.r, bias=sb.bias, s=sb.s)
        E._check(c, dict(x=x.cpu(), A=q["A"], B=q["B"], bias=q["bias"], dy=q["dy"]),
                 dict(y=ys[i].cpu(), h=hs[i].view(st.T, 64).cpu(), dA=outs[i][0].cpu(), dB=outs[i][1].cpu(),
                      dbias=None if outs[i][2] is None else outs[i][2].cpu()))
    ref, bnd = SI._dx_reference(st, types.SimpleNamespace(inp=cpu), None)
    check_bound(dxs.cpu(), ref, bnd, name="cached_groups: dX")


def test_zz_graph_coverage():
    """Every kernel a case claims appeared in the trace of its eager twin, and claims + exemptions cover every __global__ of
    the sources (the second half also runs without a GPU: tests/test_graph_plan_cpu.py)."""
    if len(TRACES) < len(GP.CASES):
        pytest.skip(f"the coverage check runs after every case ({len(TRACES)} of {len(GP.CASES)} ran)")
    seen = set()
    for case in GP.CASES:
        for k in case.claims:
            assert GR.has_kernel(TRACES[case.id], k), f"{case.id} claims {k}: {sorted(set(TRACES[case.id]))}"
            seen.add(k)
    names = GP.kernel_names()
    left = names - seen - set(GP.EXEMPT)
    assert not left, f"kernels neither replayed from a graph nor exempt: {sorted(left)}"
    print(f"{len(seen)} of {len(names)} kernels replayed from a graph, {len(GP.EXEMPT)} exempt")
