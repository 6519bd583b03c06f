"""-m gpu: the shared-input sibling kernels (sow_forward_shared / sow_backward_shared, chain2_shared.hip) and
group_siblings(model, shared_input=True).

* C ABI, forward: y_i and h_save_i bit-identical to sow_forward_group on the same x, on poisoned memory, guards intact.
* C ABI, backward: dh_i -- observed through dA (and dB, dbias) of the weight phases -- bit-identical to sow_backward_group;
  the one dX within check_bound (tests/numerics.py) of the float64 sum over the siblings of s dY_i B_i^T A_i^T, with the
  kernel's one output rounding; grad_beta = 1 accumulates onto a non-zero dX; a repeat on poisoned memory is bit-identical.
* Refusal: a set outside the admitted one returns SOW_ERR_UNSUPPORTED (differing x pointers: SOW_ERR_SHAPE) and leaves
  every output untouched.
* Modules: outputs and weight gradients bit-identical to shared_input=False, the input gradient within the bound of its
  float64 reference; FactorBucket's flat gradient bit-identical; sets the kernel does not admit behave exactly as
  shared_input=False.
"""
import copy
import dataclasses
from typing import List

import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from numerics import UNIT_ROUNDOFF, accumulation_term, bound, check_bound, fp32_floor, to64
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
GUARD = 64
SENTINEL = -7.25
DATA, WEIGHTS = _lib.BWD_DATA, _lib.BWD_WEIGHTS


def _dt(dtype):
    return {BF16: _lib.BF16, F16: _lib.F16, F32: _lib.F32}[dtype]


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Arena:
    """Guarded buffers: inputs with NaN neighbours, outputs with sentinel guards that can be poisoned before a run."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.outs = []

    def input(self, t):
        if t is None:
            return None
        n = t.numel()
        buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=self.dtype, device=DEV)
        view = buf[GUARD:GUARD + n].view(t.shape)
        view.copy_(t.to(DEV, self.dtype))
        return view

    def output(self, shape, initial=None):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=self.dtype, device=DEV)
        view = buf[GUARD:GUARD + n].view(shape)
        self.outs.append((buf, view, None if initial is None else initial.to(DEV, self.dtype)))
        return view

    def workspace(self, nbytes):
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
        self.outs.append((ws, ws, None))
        return ws

    def fill(self, byte):
        for buf, view, init in self.outs:
            if init is not None:
                view.copy_(init)
            elif buf.dtype == torch.uint8:
                buf.fill_(byte)
            else:
                _bits(view).fill_(-1 if byte == 0xFF else 0)

    def check_guards(self, what):
        torch.cuda.synchronize()
        for buf, view, _ in self.outs:
            if buf.dtype == torch.uint8:
                continue
            for name, g in (("leading", buf[:GUARD]), ("trailing", buf[-GUARD:])):
                assert not (g != SENTINEL).any(), f"{what}: {name} output guard overwritten"


@dataclasses.dataclass
class Sib:
    d_out: int
    r: int = 50
    bias: bool = False
    s: float = 0.5


@dataclasses.dataclass
class Set:
    name: str
    dtype: torch.dtype
    T: int
    d_in: int
    sibs: List[Sib]
    grad_beta: float = 0.0


SETS = [
    Set("qkv_bf16", BF16, 32768, 512, [Sib(512), Sib(512), Sib(512)]),
    Set("gqa_bf16", BF16, 32768, 512, [Sib(512, bias=True), Sib(128, 32), Sib(128, 16, s=1.0)]),
    Set("gateup_bf16", BF16, 32768, 512, [Sib(1376), Sib(1376)]),
    Set("ragged_bias_bf16", BF16, 32768 + 37, 512, [Sib(512, bias=True), Sib(264, 62, bias=True), Sib(136, 8)]),
    Set("four_bf16", BF16, 9000, 256, [Sib(256, 50, True), Sib(64, 16), Sib(64, 16), Sib(200, 4, True)]),
    Set("qkv_f16", F16, 32768, 512, [Sib(512), Sib(512), Sib(512)]),
    Set("gateup_bias_f16", F16, 32768 + 37, 512, [Sib(1376, bias=True), Sib(1376, 48, bias=True)]),
    Set("accumulate_bf16", BF16, 16384, 512, [Sib(512), Sib(256, 32)], grad_beta=1.0),
]


def _data(st: Set, seed=0):
    g = torch.Generator().manual_seed(7 + seed + st.T)
    x = torch.randn(st.T, st.d_in, generator=g)
    per = []
    for sb in st.sibs:
        A = torch.randn(st.d_in, sb.r, generator=g) / st.d_in ** 0.5
        B = torch.randn(sb.r, sb.d_out, generator=g) / sb.r ** 0.5
        bias = torch.randn(sb.d_out, generator=g) * 0.1 if sb.bias else None
        dy = torch.randn(st.T, sb.d_out, generator=g)
        per.append(dict(A=A, B=B, bias=bias, dy=dy))
    dx0 = torch.randn(st.T, st.d_in, generator=g) if st.grad_beta else None
    return x, per, dx0


class Bound:
    """The C-ABI buffers of one sibling set: shared inputs, and two complete output sets (grouped / shared)."""

    def __init__(self, st: Set, x, per, dx0):
        lib = _lib.load()
        self.st, self.ar = st, Arena(st.dtype)
        ar, dt = self.ar, _dt(st.dtype)
        zeros = (lambda shape: torch.zeros(shape)) if st.grad_beta else (lambda shape: None)   # accumulated onto
        self.x = ar.input(x)
        self.inp = [dict(A=ar.input(p["A"]), B=ar.input(p["B"]), bias=ar.input(p["bias"]), dy=ar.input(p["dy"])) for p in per]
        self.sets = {}
        for kind in ("group", "shared"):
            outs = []
            shared_dx = ar.output((st.T, st.d_in), dx0) if kind == "shared" else None
            for sb in st.sibs:
                o = dict(y=ar.output((st.T, sb.d_out)), h=ar.output((st.T, 64)),
                         dx=shared_dx if kind == "shared" else ar.output((st.T, st.d_in)),
                         dA=ar.output((st.d_in, sb.r), zeros((st.d_in, sb.r))), dB=ar.output((sb.r, sb.d_out), zeros((sb.r, sb.d_out))),
                         dbias=ar.output((sb.d_out,), zeros((sb.d_out,))) if sb.bias else None)
                o["ws"] = ar.workspace(lib.sow_workspace_bytes(st.T, st.d_in, sb.d_out, sb.r, 0, _lib.ACC_NONE, dt))
                outs.append(o)
            self.sets[kind] = outs

    def args(self, kind, h_from=None, acc=None):
        st = self.st
        arr = (_lib.LayerArgs * len(st.sibs))()
        for i, (sb, p, o) in enumerate(zip(st.sibs, self.inp, self.sets[kind])):
            h = (h_from or self.sets[kind])[i]["h"]
            arr[i] = _lib.LayerArgs(x=_ptr(self.x), A=_ptr(p["A"]), B=_ptr(p["B"]), acc_down=_ptr(acc), acc_up=None,
                                    bias=_ptr(p["bias"]), y=_ptr(o["y"]), h_save=_ptr(h), dy=_ptr(p["dy"]),
                                    dx=_ptr(o["dx"]) if (kind == "group" or i == 0) else None, dA=_ptr(o["dA"]),
                                    dB=_ptr(o["dB"]), dbias=_ptr(o["dbias"]), T=st.T, d_in=st.d_in, d_out=sb.d_out,
                                    r_live=sb.r, r_acc=0, acc_kind=_lib.ACC_DENSE if acc is not None else _lib.ACC_NONE,
                                    scale=sb.s, grad_beta=st.grad_beta if i == 0 else 0.0, workspace=_ptr(o["ws"]),
                                    workspace_bytes=o["ws"].numel())
        return arr


@pytest.mark.parametrize("st", SETS, ids=[s.name for s in SETS])
def test_shared_forward_matches_grouped(st):
    lib = _lib.load()
    x, per, _ = _data(st)
    b = Bound(st, x, per, None)
    n, dt = len(st.sibs), _dt(st.dtype)
    runs = []
    for byte in (0xFF, 0x00):
        b.ar.fill(byte)
        _lib.check(lib.sow_forward_group(b.args("group"), n, dt, _stream()), "sow_forward_group")
        _lib.check(lib.sow_forward_shared(b.args("shared"), n, dt, _stream()), "sow_forward_shared")
        b.ar.check_guards(f"{st.name} forward")
        runs.append([{k: o[k].clone() for k in ("y", "h")} for o in b.sets["shared"]])
        for i, (og, os_) in enumerate(zip(b.sets["group"], b.sets["shared"])):
            for k in ("y", "h"):
                assert torch.equal(_bits(og[k]), _bits(os_[k])), f"{st.name}: sibling {i} {k} differs from the grouped path"
    for i in range(n):
        for k in ("y", "h"):
            assert torch.equal(_bits(runs[0][i][k]), _bits(runs[1][i][k])), f"{st.name}: {k} of sibling {i} differs on a repeat"
    # h_save-free forward (no backward follows): y unchanged
    arr = b.args("shared")
    for i in range(n):
        arr[i].h_save = None
    y0 = [o["y"].clone() for o in b.sets["shared"]]
    for o in b.sets["shared"]:
        _bits(o["y"]).fill_(-1)
    _lib.check(lib.sow_forward_shared(arr, n, dt, _stream()), "sow_forward_shared")
    for i, o in enumerate(b.sets["shared"]):
        assert torch.equal(_bits(o["y"]), _bits(y0[i])), f"{st.name}: y of sibling {i} without h_save"


def _dx_reference(st: Set, b: Bound, dx0):
    """float64 sum over the siblings of dh_i A_i^T (dh_i = s dY_i B_i^T, rounded once to bf16 by the kernel: the hidden
    rounding's accumulation term), the fp32 floor of the in-kernel sum, one output ulp."""
    ref = torch.zeros(st.T, st.d_in, dtype=torch.float64)
    sq = torch.zeros_like(ref)
    n_x = 0
    for sb, p in zip(st.sibs, b.inp):
        A, B, dy = to64(p["A"]), to64(p["B"]), to64(p["dy"])
        dh = sb.s * (dy @ B.t())
        ref += dh @ A.t()
        sq += (dh * dh) @ (A * A).t()
        n_x += sb.d_out + 64
    if st.grad_beta:
        ref += st.grad_beta * to64(dx0.to(st.dtype))
    u = UNIT_ROUNDOFF[st.dtype]
    return ref, bound(ref, st.dtype, accumulation_term(sq, u, 1), fp32_floor(sq, n_x))


@pytest.mark.parametrize("st", SETS, ids=[s.name for s in SETS])
def test_shared_backward_matches_grouped_and_fp64(st):
    lib = _lib.load()
    x, per, dx0 = _data(st, seed=1)
    b = Bound(st, x, per, dx0)
    n, dt = len(st.sibs), _dt(st.dtype)
    hs = b.sets["group"]
    runs = []
    for byte in (0xFF, 0xFF):
        b.ar.fill(byte)
        _lib.check(lib.sow_forward_group(b.args("group"), n, dt, _stream()), "sow_forward_group")
        _lib.check(lib.sow_backward_group(b.args("group"), n, dt, DATA | WEIGHTS, _stream()), "sow_backward_group")
        _lib.check(lib.sow_backward_shared(b.args("shared", h_from=hs), n, dt, DATA | WEIGHTS, _stream()), "sow_backward_shared")
        b.ar.check_guards(f"{st.name} backward")
        for i, (og, os_) in enumerate(zip(b.sets["group"], b.sets["shared"])):
            for k in ("dA", "dB", "dbias"):
                if og[k] is not None:
                    assert torch.equal(og[k].view(torch.int32), os_[k].view(torch.int32)), \
                        f"{st.name}: {k} of sibling {i} differs from the grouped path (dh is not bit-identical)"
        runs.append(b.sets["shared"][0]["dx"].clone())
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), f"{st.name}: dX differs on a repeat on poisoned memory"
    dx = runs[0].cpu()
    if st.dtype == BF16:
        ref, bnd = _dx_reference(st, b, dx0)
        check_bound(dx, ref, bnd, name=f"{st.name}: dX")
    else:   # (numerics.py carries no f16 ulp model) the sum of the grouped path's dX, formed in fp64
        ref = sum(to64(o["dx"]) for o in b.sets["group"])
        assert rel_err(dx.double(), ref) < 2e-3


REFUSED = [
    ("short_T8192", BF16, 8192, {}),
    ("dense_accumulator", BF16, 32768, {"acc": True}),
    ("rank100", BF16, 32768, {"r": 100}),
    ("fp32", F32, 32768, {}),
    ("differing_x", BF16, 32768, {"other_x": True}),
    ("switch_NO_SHARED_X", BF16, 32768, {"switch": True}),
]


@pytest.mark.parametrize("name,dtype,T,how", REFUSED, ids=[r[0] for r in REFUSED])
def test_shared_refuses_outside_the_admitted_set(name, dtype, T, how):
    lib = _lib.load()
    r = how.get("r", 50)
    st = Set(name, dtype, T, 512, [Sib(512, r), Sib(512, r), Sib(256, r)])
    x, per, _ = _data(st)
    b = Bound(st, x, per, None)
    acc = b.ar.input(torch.randn(512, 512) * 0.01) if how.get("acc") else None
    n, dt = len(st.sibs), _dt(dtype)
    b.ar.fill(0x00)
    fwd, bwd = b.args("shared", acc=acc), b.args("shared", acc=acc)
    if how.get("other_x"):
        other = b.ar.input(x)
        fwd[1].x = bwd[1].x = other.data_ptr()
    snap = [{k: (None if o[k] is None else o[k].clone()) for k in ("y", "h", "dx", "dA", "dB", "dbias")}
            for o in b.sets["shared"]]
    want = _lib.ERR_SHAPE if how.get("other_x") else _lib.ERR_UNSUPPORTED
    if how.get("switch"):
        with _lib.switch(NO_SHARED_X=1):
            rcs = (lib.sow_forward_shared(fwd, n, dt, _stream()), lib.sow_backward_shared(bwd, n, dt, DATA | WEIGHTS, _stream()))
    else:
        rcs = (lib.sow_forward_shared(fwd, n, dt, _stream()), lib.sow_backward_shared(bwd, n, dt, DATA | WEIGHTS, _stream()))
    assert rcs == (want, want), rcs
    b.ar.check_guards(name)
    for o, s in zip(b.sets["shared"], snap):
        for k, v in s.items():
            if v is not None:
                assert torch.equal(_bits(o[k]) if o[k].dtype != F32 else o[k].view(torch.int32),
                                   _bits(v) if v.dtype != F32 else v.view(torch.int32)), f"{name}: {k} was written"


# ---------------------------------------------------------------------------------------------------------------- modules
class _Heads(nn.Module):
    """q / k / v on one input and gate / up on another, with HF names; the loss weights every output with a fixed tensor,
    so that no sibling's weight gradient depends on another group's input gradient."""

    def __init__(self, d=512, inter=1376, r=50, dtype=BF16, bias=False, kv=512):
        super().__init__()
        from sow_amd import SoWLinear
        mk = lambda i, o, rr=r: SoWLinear(i, o, bias=bias, rank=rr, init_method="normal", scale=0.5, device=DEV, dtype=dtype)
        self.self_attn, self.mlp = nn.Module(), nn.Module()
        self.self_attn.q_proj, self.self_attn.k_proj, self.self_attn.v_proj = mk(d, d), mk(d, kv), mk(d, kv)
        self.mlp.gate_proj, self.mlp.up_proj = mk(d, inter), mk(d, inter)

    def forward(self, x, x2, w):
        a = self.self_attn
        outs = [a.q_proj(x), a.k_proj(x), a.v_proj(x), self.mlp.gate_proj(x2), self.mlp.up_proj(x2)]
        return sum((o.float() * wi).sum() for o, wi in zip(outs, w)), outs


def _inputs_for(net, T, d=512, seed=3, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, d, generator=g).to(DEV, dtype).requires_grad_(True)
    x2 = torch.randn(T, d, generator=g).to(DEV, dtype).requires_grad_(True)
    mods = [net.self_attn.q_proj, net.self_attn.k_proj, net.self_attn.v_proj, net.mlp.gate_proj, net.mlp.up_proj]
    w = [torch.randn(T, m.out_features, generator=g).to(DEV) for m in mods]
    return x, x2, w


def _run(net, x, x2, w, no_grad=False, reset=True):
    for p in net.parameters():
        if reset:
            p.grad = None
    x, x2 = x.detach().clone().requires_grad_(not no_grad), x2.detach().clone().requires_grad_(not no_grad)
    if no_grad:
        with torch.no_grad():
            loss, outs = net(x, x2, w)
        return loss, outs, None
    loss, outs = net(x, x2, w)
    loss.backward()
    return loss, outs, (x.grad, x2.grad)


def _pair(**kw):
    from sow_amd import group_siblings
    base = _Heads(**kw)
    twin = copy.deepcopy(base)
    assert group_siblings(base) == 2 and group_siblings(twin, shared_input=True) == 2
    return base, twin


def test_module_shared_input_bit_identical_outputs_and_weight_grads():
    torch.manual_seed(11)
    base, twin = _pair()
    x, x2, w = _inputs_for(base, 9000)
    lb, ob, gb = _run(base, x, x2, w)
    lt, ot, gt = _run(twin, x, x2, w)
    assert torch.equal(lb, lt)
    for a, c in zip(ob, ot):
        assert torch.equal(_bits(a.detach()), _bits(c.detach()))
    for (n1, p1), (_, p2) in zip(base.named_parameters(), twin.named_parameters()):
        assert (p1.grad is None) == (p2.grad is None), n1
        if p1.grad is not None:
            assert torch.equal(_bits(p1.grad), _bits(p2.grad)), n1
    # the input gradients: one rounding of the fp32 sum, within the bound of the float64 reference
    st_x = Set("module_x", BF16, 9000, 512, [Sib(512), Sib(512), Sib(512)])
    for xg, mods, ws in ((gt[0], [twin.self_attn.q_proj, twin.self_attn.k_proj, twin.self_attn.v_proj], w[:3]),
                         (gt[1], [twin.mlp.gate_proj, twin.mlp.up_proj], w[3:])):
        ref = torch.zeros(9000, 512, dtype=torch.float64)
        sq = torch.zeros_like(ref)
        n_x = 0
        for m, wi in zip(mods, ws):
            A, B = to64(m.downscale_weights[0].data), to64(m.upscale_weights[0].data)
            dh = m.scale * (to64(wi.to(BF16)) @ B.t())
            ref += dh @ A.t()
            sq += (dh * dh) @ (A * A).t()
            n_x += m.out_features + 64
        u = UNIT_ROUNDOFF[BF16]
        check_bound(xg.cpu(), ref, bound(ref, BF16, accumulation_term(sq, u, 1), fp32_floor(sq, n_x)), name="module dX")
    for a, c in zip(gb, gt):
        assert rel_err(c.float().cpu(), a.float().cpu()) < 2e-2


def test_module_shared_input_no_grad_and_unadmitted_sets_unchanged():
    torch.manual_seed(12)
    for kw, T, admitted in (({}, 9000, True), ({}, 8192, False), ({"r": 100}, 9000, False), ({"bias": True}, 9000, True)):
        base, twin = _pair(**kw)
        x, x2, w = _inputs_for(base, T)
        lb, ob, _ = _run(base, x, x2, w, no_grad=True)
        lt, ot, _ = _run(twin, x, x2, w, no_grad=True)
        assert torch.equal(lb, lt) and all(torch.equal(_bits(a), _bits(c)) for a, c in zip(ob, ot)), kw
        if admitted:
            continue   # the backward of an admitted set: test_module_shared_input_bit_identical_outputs_and_weight_grads
        lb, ob, gb = _run(base, x, x2, w)
        lt, ot, gt = _run(twin, x, x2, w)
        assert torch.equal(lb, lt), kw
        for a, c in zip(gb, gt):   # not admitted: the grouped path, input gradients included
            assert torch.equal(_bits(a), _bits(c)), kw
        for (n1, p1), (_, p2) in zip(base.named_parameters(), twin.named_parameters()):
            if p1.grad is not None:
                assert torch.equal(_bits(p1.grad), _bits(p2.grad)), (n1, kw)
    # dense accumulator ("keep") layers and fp32 parameters under autocast: the grouped path, bit for bit
    base, twin = _pair()
    acc = torch.randn(512, 512, device=DEV, dtype=BF16) * 0.01
    for net in (base, twin):
        for m in (net.self_attn.q_proj, net.self_attn.k_proj, net.self_attn.v_proj):
            m.acc_downweight = nn.Parameter(acc.clone(), requires_grad=False)
    x, x2, w = _inputs_for(base, 9000)
    lb, ob, gb = _run(base, x, x2, w)
    lt, ot, gt = _run(twin, x, x2, w)
    assert torch.equal(lb, lt) and torch.equal(_bits(gb[0]), _bits(gt[0]))
    base, twin = _pair(dtype=F32)
    x, x2, w = _inputs_for(base, 9000, dtype=F32)
    with torch.autocast("cuda", dtype=BF16):
        lb, ob, gb = _run(base, x, x2, w)
        lt, ot, gt = _run(twin, x, x2, w)
    assert torch.equal(lb, lt) and torch.equal(gb[0].view(torch.int32), gt[0].view(torch.int32))
    for (n1, p1), (_, p2) in zip(base.named_parameters(), twin.named_parameters()):
        if p1.grad is not None:
            assert torch.equal(p1.grad.view(torch.int32), p2.grad.view(torch.int32)), n1


def test_factor_bucket_with_shared_siblings():
    from sow_amd.dp import FactorBucket, factor_parameters
    torch.manual_seed(13)
    base, twin = _pair()
    x, x2, w = _inputs_for(base, 9000)
    flats, xgs = [], []
    for net in (base, twin):
        bucket = FactorBucket(factor_parameters(net))
        assert bucket.attach(net) == 5
        bucket.zero_grad()
        _, _, g = _run(net, x, x2, w, reset=False)
        bucket.finalize()
        torch.cuda.synchronize()
        flats.append(bucket.flat_grad.clone())
        xgs.append(g)
    assert torch.equal(flats[0].view(torch.int16), flats[1].view(torch.int16))
    for a, c in zip(*xgs):
        assert rel_err(c.float().cpu(), a.float().cpu()) < 2e-2


def test_group_siblings_shared_in_a_llama_block():
    """A tiny Llama (T = 8 x 1100 tokens > 8192) with shared_input=True: the loss is bit-identical to shared_input=False; the
    parameters that no shared input gradient reaches (lm_head, the final norm, the MLP of the last block) get bit-identical
    gradients; the others, downstream of a once-rounded dX in backward, agree to bf16 rounding."""
    transformers = pytest.importorskip("transformers")
    from sow_amd import SoWConfig, group_siblings, prepare_sow
    torch.manual_seed(7)
    cfg = transformers.LlamaConfig(hidden_size=128, intermediate_size=344, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, vocab_size=256, max_position_embeddings=1100, rms_norm_eps=1e-6,
                                   tie_word_embeddings=False, attn_implementation="eager")
    base = transformers.AutoModelForCausalLM.from_config(cfg)
    base = prepare_sow(base, SoWConfig(target_modules=["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"],
                                       rank=8, init_method="normal", scale=0.5, device="cpu"))
    base = base.to(DEV, BF16)
    twin = copy.deepcopy(base)
    assert group_siblings(base) == 4 and group_siblings(twin, shared_input=True) == 4
    tokens = torch.randint(0, 256, (8, 1100), generator=torch.Generator().manual_seed(1)).to(DEV)
    for net in (base, twin):
        net.zero_grad(set_to_none=True)
        loss = net(input_ids=tokens, labels=tokens.clone()).loss
        loss.backward()
        net._loss = loss.detach()
    assert torch.equal(base._loss, twin._loss)
    exact = ("lm_head", "model.norm", "layers.1.mlp")
    for (n1, p1), (_, p2) in zip(base.named_parameters(), twin.named_parameters()):
        if p1.grad is None:
            assert p2.grad is None, n1
        elif any(e in n1 for e in exact):
            assert torch.equal(_bits(p1.grad), _bits(p2.grad)), n1
        else:
            assert rel_err(p2.grad.float().cpu(), p1.grad.float().cpu()) < 2e-2, n1
