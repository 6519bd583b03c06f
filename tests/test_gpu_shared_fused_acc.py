"""-m gpu: the shared-input data gradient of siblings that carry a low-rank accumulator (sow_backward_shared under
SOW_FUSE_ACC, chain_shared_acc.hip) and group_siblings(model, shared_input=True) on such layers.

* C ABI: DATA | WEIGHTS returns SOW_OK on each case of shared_fused_acc_numerics.CASES; dA, dB and dbias -- that is, every
  dh_i the weight phases read -- bit-identical to sow_backward_group with the flagged dtype; the ONE dX within the float64
  single-rounding bound; a repeat on 0xFF-poisoned outputs and workspaces bit-identical; guards intact; a NaN in one row of
  one dY makes only that row of dX non-finite; the kernel trace shows chain_shared_acc_kernel and no chain_wide_acc_kernel.
* Refusals (unflagged dtype, the NO_FUSED_ACC and NO_SHARED_X switches, a mixed set, sow_forward_shared) return
  SOW_ERR_UNSUPPORTED and leave every output and workspace untouched.
* Modules at T = 32769, where the module surface passes the flag: SharedInputGroup.backward returns True; outputs and
  weight gradients bit-identical to shared_input=False, the input gradients within the float64 bound; FactorBucket's flat
  gradient bit-identical.  At T = 8257 nothing is admitted and everything, dX included, is the grouped path bit for bit.
"""
import copy

import pytest
import torch
import torch.nn as nn

import shared_fused_acc_numerics as SN
import test_gpu_elementwise as E
import test_gpu_shared_input as SI
from sow_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
DATA, WEIGHTS = _lib.BWD_DATA, _lib.BWD_WEIGHTS
LOWRANK = _lib.ACC_LOWRANK
_bits, _ptr, _stream = SI._bits, SI._ptr, SI._stream
_MEMO = {}


def _case_data(st):
    if st.name not in _MEMO:
        _MEMO[st.name] = SN.inputs(st)
    return _MEMO[st.name]


def _flag(st):
    return SI._dt(st.dtype) | _lib.FUSE_ACC


def _has_bias(st, i):
    return i == 0          # the first sibling of every case: r < 64 (ones column) and r = 64 (its own column sum)


class Bound:
    """The C-ABI buffers of one case: shared inputs, and two complete output sets (grouped / shared), every workspace of
    the flagged plan's size."""

    def __init__(self, st, d):
        lib = _lib.load()
        self.st, self.ar = st, SI.Arena(st.dtype)
        ar, flag = self.ar, _flag(st)
        zeros = (lambda shape: torch.zeros(shape)) if st.grad_beta else (lambda shape: None)   # accumulated onto
        g = torch.Generator().manual_seed(5)
        self.x = ar.input(d["x"])
        self.inp = []
        for i, (sb, p) in enumerate(zip(st.sibs, d["sibs"])):
            q = {k: ar.input(p[k]) for k in ("A", "B", "Q", "R", "dy")}
            q["bias"] = ar.input(torch.randn(sb.d_out, generator=g) * 0.1) if _has_bias(st, i) else None
            self.inp.append(q)
        self.sets = {}
        for kind in ("group", "shared"):
            outs = []
            shared_dx = ar.output((st.T, st.d_in), d["dx0"]) if kind == "shared" else None
            for i, sb in enumerate(st.sibs):
                o = dict(y=ar.output((st.T, sb.d_out)), h=ar.output((st.T, 64)),
                         dx=shared_dx if kind == "shared" else ar.output((st.T, st.d_in)),
                         dA=ar.output((st.d_in, sb.r), zeros((st.d_in, sb.r))), dB=ar.output((sb.r, sb.d_out), zeros((sb.r, sb.d_out))),
                         dbias=ar.output((sb.d_out,), zeros((sb.d_out,))) if _has_bias(st, i) else None)
                o["ws"] = ar.workspace(lib.sow_workspace_bytes(st.T, st.d_in, sb.d_out, sb.r, sb.r_acc, LOWRANK, flag))
                outs.append(o)
            self.sets[kind] = outs

    def args(self, kind, h_from=None):
        st = self.st
        arr = (_lib.LayerArgs * len(st.sibs))()
        for i, (sb, p, o) in enumerate(zip(st.sibs, self.inp, self.sets[kind])):
            h = (h_from or self.sets[kind])[i]["h"]
            arr[i] = _lib.LayerArgs(x=_ptr(self.x), A=_ptr(p["A"]), B=_ptr(p["B"]), acc_down=_ptr(p["Q"]), acc_up=_ptr(p["R"]),
                                    bias=_ptr(p["bias"]), y=_ptr(o["y"]), h_save=_ptr(h), dy=_ptr(p["dy"]),
                                    dx=_ptr(o["dx"]) if (kind == "group" or i == 0) else None, dA=_ptr(o["dA"]),
                                    dB=_ptr(o["dB"]), dbias=_ptr(o["dbias"]), T=st.T, d_in=st.d_in, d_out=sb.d_out,
                                    r_live=sb.r, r_acc=sb.r_acc, acc_kind=LOWRANK, scale=sb.s,
                                    grad_beta=st.grad_beta if i == 0 else 0.0, workspace=_ptr(o["ws"]),
                                    workspace_bytes=o["ws"].numel())
        return arr

    def snapshot(self):
        return [{k: (None if o[k] is None else o[k].clone()) for k in ("y", "h", "dx", "dA", "dB", "dbias", "ws")}
                for o in self.sets["shared"]]

    def assert_untouched(self, snap, what):
        self.ar.check_guards(what)
        for i, (o, s) in enumerate(zip(self.sets["shared"], snap)):
            for k, v in s.items():
                if v is not None:
                    same = torch.equal(o[k], v) if v.dtype == torch.uint8 else torch.equal(_bits(o[k]), _bits(v))
                    assert same, f"{what}: {k} of sibling {i} was written"


@pytest.mark.parametrize("st", SN.CASES, ids=lambda st: st.name)
def test_shared_backward_lowrank_matches_grouped_and_fp64(st):
    lib = _lib.load()
    d = _case_data(st)
    assert ops.shared_fused_acc_admits(st.T, st.d_in, [(sb.d_out, sb.r, sb.r_acc, LOWRANK) for sb in st.sibs], st.dtype)
    b = Bound(st, d)
    n, flag = len(st.sibs), _flag(st)
    hs = b.sets["group"]
    runs = []
    for _ in range(2):
        b.ar.fill(0xFF)
        _lib.check(lib.sow_forward_group(b.args("group"), n, flag, _stream()), "sow_forward_group")
        _lib.check(lib.sow_backward_group(b.args("group"), n, flag, DATA | WEIGHTS, _stream()), "sow_backward_group")
        rc = lib.sow_backward_shared(b.args("shared", h_from=hs), n, flag, DATA | WEIGHTS, _stream())
        assert rc == 0, f"{st.name}: sow_backward_shared returned {rc}"      # SOW_OK (without the route: -6)
        b.ar.check_guards(f"{st.name} backward")
        for i, (og, os_) in enumerate(zip(b.sets["group"], b.sets["shared"])):
            for k in ("dA", "dB", "dbias"):
                if og[k] is not None:
                    assert torch.equal(_bits(og[k]), _bits(os_[k])), \
                        f"{st.name}: {k} of sibling {i} differs from the grouped path (dh is not bit-identical)"
        runs.append(b.sets["shared"][0]["dx"].clone())
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{st.name}: dX differs on a repeat on poisoned memory"
    stats = SN.check_dx(st, d, runs[0].cpu())
    print(f"{st.name}: dX worst err / bound = {stats['worst']:.3f}")

    # ---- the kernels of the data phase: the shared kernel, no per-sibling fused pass
    b.ar.fill(0xFF)
    seq = E._kernel_seq(lambda: _lib.check(lib.sow_backward_shared(b.args("shared", h_from=hs), n, flag, DATA, _stream()),
                                           "sow_backward_shared"))
    assert any("chain_shared_acc_kernel" in k for k in seq) and not any("chain_wide_acc_kernel" in k for k in seq), seq
    assert torch.equal(_bits(b.sets["shared"][0]["dx"]), _bits(runs[0])), f"{st.name}: dX of a DATA-only call"

    # ---- a NaN in one row of one dY reaches that row of dX and no other
    row, sib = st.T - 3, n - 1
    dy = b.inp[sib]["dy"]
    keep = dy[row, 1].clone()
    dy[row, 1] = float("nan")
    b.ar.fill(0xFF)
    _lib.check(lib.sow_backward_shared(b.args("shared", h_from=hs), n, flag, DATA, _stream()), "sow_backward_shared")
    bad = ~torch.isfinite(b.sets["shared"][0]["dx"].float()).all(dim=1)
    dy[row, 1] = keep
    assert bad.nonzero().flatten().tolist() == [row], f"{st.name}: non-finite rows of dX {bad.nonzero().flatten().tolist()[:8]}"
    b.ar.check_guards(f"{st.name} NaN row")


REFUSED = ["unflagged", "NO_FUSED_ACC", "NO_SHARED_X", "mixed_set", "forward"]


@pytest.mark.parametrize("how", REFUSED)
def test_refusals_leave_every_output_untouched(how):
    lib = _lib.load()
    st = SN.CASES[0]
    b = Bound(st, _case_data(st))
    n, flag = len(st.sibs), _flag(st)
    b.ar.fill(0x00)
    arr = b.args("shared")
    snap = b.snapshot()
    if how == "unflagged":
        rc = lib.sow_backward_shared(arr, n, SI._dt(st.dtype), DATA | WEIGHTS, _stream())
    elif how in ("NO_FUSED_ACC", "NO_SHARED_X"):
        with _lib.switch(**{how: 1}):
            rc = lib.sow_backward_shared(arr, n, flag, DATA | WEIGHTS, _stream())
    elif how == "mixed_set":
        arr[1].acc_kind, arr[1].r_acc, arr[1].acc_down, arr[1].acc_up = _lib.ACC_NONE, 0, None, None
        rc = lib.sow_backward_shared(arr, n, flag, DATA | WEIGHTS, _stream())
    else:
        rc = lib.sow_forward_shared(arr, n, flag, _stream())
    assert rc == _lib.ERR_UNSUPPORTED, (how, rc)
    b.assert_untouched(snap, how)


# ---------------------------------------------------------------------------------------------------------------- modules
HID, INTER, R, R_ACC = 128, 264, 8, 24


def _lowrank_pair(r_acc=R_ACC):
    """_Heads of low-rank-accumulator layers: grouped (base) and shared-input grouped (twin), the same parameters."""
    from sow_amd import group_siblings
    torch.manual_seed(21)
    base = SI._Heads(d=HID, inter=INTER, r=R, kv=HID)
    g = torch.Generator().manual_seed(22)
    for m in _mods(base):
        m.acc_downweight = nn.Parameter((torch.randn(m.in_features, r_acc, generator=g) * 0.05).to(DEV, BF16), requires_grad=False)
        m.acc_upweight = nn.Parameter((torch.randn(r_acc, m.out_features, generator=g) * 0.05).to(DEV, BF16), requires_grad=False)
    twin = copy.deepcopy(base)
    assert group_siblings(base) == 2 and group_siblings(twin, shared_input=True) == 2
    return base, twin


def _mods(net):
    return [net.self_attn.q_proj, net.self_attn.k_proj, net.self_attn.v_proj, net.mlp.gate_proj, net.mlp.up_proj]


@pytest.fixture
def shared_rc(monkeypatch):
    """What every SharedInputGroup.backward of the test returned."""
    rcs, orig = [], ops.SharedInputGroup.backward

    def backward(grp, *a, **k):
        rc = orig(grp, *a, **k)
        rcs.append(rc)
        return rc

    monkeypatch.setattr(ops.SharedInputGroup, "backward", backward)
    return rcs


def _assert_same_outputs_and_weight_grads(base, twin, lb, lt, ob, ot):
    assert torch.equal(lb, lt)
    for a, c in zip(ob, ot):
        assert torch.equal(_bits(a.detach()), _bits(c.detach()))
    for (n1, p1), (_, p2) in zip(base.named_parameters(), twin.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), n1
        if p1.grad is not None:
            assert torch.equal(_bits(p1.grad), _bits(p2.grad)), n1


def _module_set(mods, ws, T, name):
    """The SN.Set and its inputs of one sibling group of the module: dY_i = the loss weights, cast to bf16 by autograd."""
    st = SN.Set(name, BF16, T, HID, [SN.Sib(m.out_features, R, m.acc_downweight.shape[1], s=float(m.scale)) for m in mods])
    d = dict(x=None, dx0=None, sibs=[dict(A=m.downscale_weights[0].data.cpu(), B=m.upscale_weights[0].data.cpu(),
                                          Q=m.acc_downweight.data.cpu(), R=m.acc_upweight.data.cpu(), dy=wi.to(BF16).cpu())
                                     for m, wi in zip(mods, ws)])
    return st, d


def test_module_shared_input_lowrank_takes_the_shared_route(shared_rc):
    T = 32769
    base, twin = _lowrank_pair()
    assert all(ops.fuse_acc_default(T, HID, m.out_features, R, R_ACC, LOWRANK, BF16) for m in _mods(base))
    x, x2, w = SI._inputs_for(base, T, d=HID)
    lb, ob, gb = SI._run(base, x, x2, w)
    assert shared_rc == []
    lt, ot, gt = SI._run(twin, x, x2, w)
    assert shared_rc == [True, True], shared_rc
    _assert_same_outputs_and_weight_grads(base, twin, lb, lt, ob, ot)
    for xg, mods, ws, name in ((gt[0], _mods(twin)[:3], w[:3], "module qkv"), (gt[1], _mods(twin)[3:], w[3:], "module gate_up")):
        st, d = _module_set(mods, ws, T, name)
        SN.check_dx(st, d, xg.cpu())
    for a, c in zip(gb, gt):
        assert SI.rel_err(c.float().cpu(), a.float().cpu()) < 2e-2


def test_module_keeps_the_grouped_path_where_the_shared_kernel_measured_slower(shared_rc):
    """r_acc + r = 192: q / k / v plan 104 KiB of LDS (one workgroup per CU: ops.shared_fused_acc_pays says no, the grouped
    path runs and its dX comes back bit for bit), gate / up plan 80 KiB (two per CU: the shared route)."""
    T, r_acc = 32769, 192 - R
    assert not ops.shared_fused_acc_pays([192] * 3) and ops.shared_fused_acc_pays([192] * 2)
    base, twin = _lowrank_pair(r_acc)
    x, x2, w = SI._inputs_for(base, T, d=HID)
    lb, ob, gb = SI._run(base, x, x2, w)
    lt, ot, gt = SI._run(twin, x, x2, w)
    assert sorted(shared_rc) == [False, True], shared_rc
    _assert_same_outputs_and_weight_grads(base, twin, lb, lt, ob, ot)
    assert torch.equal(_bits(gb[0]), _bits(gt[0]))
    st, d = _module_set(_mods(twin)[3:], w[3:], T, "module gate_up r_pad 192")
    SN.check_dx(st, d, gt[1].cpu())
    # the C ABI itself admits the larger set: the rule belongs to the module surface
    assert ops.shared_fused_acc_admits(T, HID, [(HID, R, r_acc, LOWRANK)] * 3, BF16)


def test_factor_bucket_with_shared_lowrank_siblings(shared_rc):
    from sow_amd.dp import FactorBucket, factor_parameters
    T = 32769
    base, twin = _lowrank_pair()
    x, x2, w = SI._inputs_for(base, T, d=HID)
    flats, xgs = [], []
    for net in (base, twin):
        bucket = FactorBucket(factor_parameters(net))
        assert bucket.attach(net) == 5
        bucket.zero_grad()
        _, _, g = SI._run(net, x, x2, w, reset=False)
        bucket.finalize()
        torch.cuda.synchronize()
        flats.append(bucket.flat_grad.clone())
        xgs.append(g)
    assert shared_rc == [True, True], shared_rc
    assert torch.equal(_bits(flats[0]), _bits(flats[1]))
    for xg, mods, ws, name in ((xgs[1][0], _mods(twin)[:3], w[:3], "bucket qkv"), (xgs[1][1], _mods(twin)[3:], w[3:], "bucket gate_up")):
        st, d = _module_set(mods, ws, T, name)
        SN.check_dx(st, d, xg.cpu())


def test_module_shared_input_lowrank_below_the_flag_is_the_grouped_path(shared_rc):
    T = 8257
    base, twin = _lowrank_pair()
    x, x2, w = SI._inputs_for(base, T, d=HID)
    lb, ob, gb = SI._run(base, x, x2, w)
    lt, ot, gt = SI._run(twin, x, x2, w)
    assert shared_rc == [False, False], shared_rc
    _assert_same_outputs_and_weight_grads(base, twin, lb, lt, ob, ot)
    for a, c in zip(gb, gt):
        assert torch.equal(_bits(a), _bits(c))
