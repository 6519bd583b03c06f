"""-m gpu: the batched tensor-train kernels of sow_amd/csrc/tt_batch.hip (sow_tt_reconstruct_batch, sow_tt_decompose_batch,
sow_ttadam_batch), element by element against float64 (tests/tt_numerics.py), through the C ABI.

As test_gpu_step_elementwise.py: inputs are views into buffers whose neighbours (and row gaps, for pitched operands) hold
NaN, every core / matrix / parameter output sits between sentinel guards, outputs and workspaces are poisoned with 0xFF
bytes, then zeroed, then poisoned again, and the three runs must agree bit for bit (no atomics in these kernels; in-place
cores and p are restored before each run).  Every workspace is exactly sow_*_workspace_bytes long inside a larger
sentinel-filled byte buffer whose other bytes must survive.  The -s output lists the worst err / limit of every check.
"""
import ctypes
import math
import random

import pytest
import torch

import test_gpu_step_elementwise as SE
import tt_numerics as T
from numerics import NumericsError, check_bound, to64, ulp
from step_numerics import C_QR, U32
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
WS_SENTINEL = 0xA5
WS_PAD = 320                 # bytes on both sides of a workspace; the start is odd on purpose (the kernels align it)
WORST = {}                   # check kind -> (worst err / limit, case)
LAPACK_STAGES = [0, 0]       # decomposition stages compared with LAPACK, stages in all


def _f(x):
    return float(torch.tensor(x, dtype=torch.float64).float())


class Arena(SE.Arena):
    """SE.Arena plus exact-size workspaces inside sentinel-filled byte buffers, and pitched views whose row gaps hold the
    sentinel (outputs) or NaN (inputs)."""

    def __init__(self):
        super().__init__()
        self.wss = []
        self.gaps = []       # views of the gap columns of pitched outputs

    def workspace(self, nbytes):
        buf = torch.full((nbytes + 2 * WS_PAD + 1,), WS_SENTINEL, dtype=torch.uint8, device=DEV)
        self.wss.append((buf, WS_PAD + 1, nbytes))
        return buf.data_ptr() + WS_PAD + 1

    def fill(self, byte):
        super().fill(byte)
        for buf, off, n in self.wss:
            buf[off:off + n].fill_(byte)
        for gap in self.gaps:
            gap.fill_(SE.SENTINEL)

    def check_guards(self, what):
        super().check_guards(what)
        for buf, off, n in self.wss:
            assert (buf[:off] == WS_SENTINEL).all() and (buf[off + n:] == WS_SENTINEL).all(), \
                f"{what}: a byte outside a workspace of exactly the queried size was written"
        for gap in self.gaps:
            assert not (gap != SE.SENTINEL).any(), f"{what}: the row gap of a pitched output was written"

    def pitched_input(self, mat, extra):
        if not extra:
            return self.input(mat), mat.shape[1]
        full = torch.cat([mat, torch.full((mat.shape[0], extra), float("nan"), dtype=mat.dtype)], 1)
        return self.input(full)[:, :mat.shape[1]], mat.shape[1] + extra

    def pitched_output(self, rows, cols, extra, initial=None):
        """The [rows, cols] view of a [rows, cols + extra] output and its pitch; `initial` is restored before every run."""
        if initial is not None and extra:
            initial = torch.cat([initial, torch.full((rows, extra), SE.SENTINEL, dtype=F32)], 1)
        buf = self.output((rows, cols + extra), F32, initial=initial)
        if extra:
            self.gaps.append(buf[:, cols:])
        return buf[:, :cols], cols + extra


def _desc(core_views, spec):
    rows, cols, ranks, ind, outd = spec
    d = _lib.TtDesc()
    d.order = len(ind)
    for k in range(min(len(ind), _lib.TT_MAX_ORDER)):
        d.cores[k], d.in_dims[k], d.out_dims[k] = core_views[k].data_ptr(), ind[k], outd[k]
    for k, r in enumerate(ranks[:_lib.TT_MAX_ORDER + 1]):
        d.ranks[k] = r
    d.rows, d.cols = rows, cols
    return d


def _note(case, stats):
    parts = []
    for k, s in stats.items():
        if "counted" in s:
            LAPACK_STAGES[0] += s["counted"]
            LAPACK_STAGES[1] += s["stages"]
        if s["worst"] > WORST.get(k, (-1.0, ""))[0]:
            WORST[k] = (s["worst"], case)
        parts.append(f"{k} {s['worst']:.3g}" + (f" [{s['counted']}/{s['stages']}]" if "counted" in s else "")
                     + (f" (undecided {100 * s['undecided']:.3f} %)" if "undecided" in s else ""))
    print(f"{case}: " + ", ".join(parts))


def _fold(into, stats):
    for k, s in stats.items():
        if k not in into or s["worst"] > into[k]["worst"]:
            keep = into.get(k, {})
            into[k] = dict(s)
            for c in ("counted", "stages"):
                if c in s:
                    into[k][c] = s[c] + keep.get(c, 0)
        elif "counted" in s:
            into[k]["counted"] += s["counted"]
            into[k]["stages"] += s["stages"]


# ---- shapes ------------------------------------------------------------------------------------------------------------
def spec(rows, cols, ranks, ind=None, outd=None):
    if ind is None:
        ind, outd = T.default_dims(rows, cols, len(ranks) - 1)
    return (rows, cols, list(ranks), list(ind), list(outd))


S = dict(
    o1=spec(37, 5, [1, 1], [37], [5]),                                      # order 1: the copy path of decompose_stages
    o1_pad=spec(37, 5, [1, 1], [40], [8]),
    o2_r3=spec(37, 5, [1, 3, 1]),                                           # 7x7 / 3x3 modes: padded both ways
    o2_r16=spec(100, 60, [1, 16, 1]),
    o2_big=spec(768, 3072, [1, 16, 1]),                                     # rest = 3120 >= 512, m = 1568 = 24.5 x 64
    o2_full=spec(30, 28, [1, 30, 1], [6, 5], [5, 6]),                       # r_1 = m = 30: no truncation
    o3_r8=spec(512, 512, [1, 8, 8, 1]),                                     # exact; rest = 4088 and 56
    o3_r16=spec(200, 90, [1, 16, 16, 1], [6, 6, 6], [5, 5, 4]),             # tt_eval<32> inner bond; in != out
    o3_r32=spec(512, 1376, [1, 32, 32, 1]),                                 # rank at the limit
    o3_r9=spec(60, 50, [1, 9, 8, 1], [4, 1, 16], [5, 11, 1]),               # 1-wide modes
    o3_kc=spec(30, 20, [1, 32, 32, 1], [8, 2, 2], [6, 2, 2]),               # kc < r at both bonds
    o4_r4=spec(81, 81, [1, 4, 4, 4, 1]),                                    # exact
    o4_kc=spec(20, 12, [1, 6, 12, 12, 1], [5, 2, 2, 1], [3, 2, 1, 2]),
    o5=spec(30, 30, [1, 4, 8, 8, 4, 1], [2] * 5, [2] * 5),
    o6=spec(60, 40, [1, 4, 6, 8, 6, 4, 1], [2] * 6, [2] * 6),
    o3_nc1=spec(14, 9, [1, 6, 2, 1], [3, 5, 1], [3, 3, 1]),                 # last bond: ncols = 1 < r = 2, kc = 1, rest = 0
    o3_rest1=spec(33, 5, [1, 6, 2, 1], [4, 3, 3], [3, 2, 1]),               # last bond: ncols = 3, kc = 2: rest = 1 (wave branch)
    o4_rest1=spec(55, 28, [1, 4, 8, 4, 1], [3, 2, 2, 5], [2, 3, 5, 1]),     # last bond: ncols = 5, kc = 4: rest = 1, m = 80
)


def features(batch, chunk, evaluated=None):
    """What a batch reaches, from its shapes alone.  `chunk`: trains (16, reconstruct / decompose) or items (8, TTAdam) per
    launch: the tt_eval template is picked from the largest rank of a launch chunk.  `evaluated`: per train, whether tt_eval
    runs on it at all (reconstruct: always; sow_ttadam_batch: only for items with state)."""
    f = set()
    if len({len(s[3]) for s in batch}) > 1:
        f.add("mixed_order")
    for i, s in enumerate(batch):
        rows, cols, ranks, ind, outd = s
        d = len(ind)
        if d == 1:
            f.add("order1")
        base = i - i % chunk
        maxr = max(max(t[2]) for t in batch[base:base + chunk])
        if d >= 2 and (evaluated is None or evaluated[i]):
            f.add("eval8" if maxr <= 8 else "eval32")
            if maxr > 8 and any(ranks[k] > 8 and ranks[k + 1] > 1 for k in range(1, d)):
                f.add("eval32_inner")
        for m, nc, kc, r in T.stage_shapes(ranks, ind, outd):
            if nc - kc >= 512:
                f.add("rrest_wide")
            elif nc - kc > 0:
                f.add("rrest_wave")
            if nc - kc == 1:
                f.add("rest=1")
            if kc < r:
                f.add("kc<r")
            if r == m:
                f.add("full_rank")
    return f


# ---- reconstruct / decompose -------------------------------------------------------------------------------------------
def _gauss(rows, cols, gen):
    return torch.randn(rows, cols, generator=gen, dtype=torch.float64).float()


def _low_rank_kron(gen):
    """A sum of three Kronecker products of 8 x 8 factors: TT rank 3 at order 2, which a rank-16 train must reproduce."""
    return sum(torch.kron(torch.randn(8, 8, generator=gen, dtype=torch.float64), torch.randn(8, 8, generator=gen, dtype=torch.float64))
               for _ in range(3)).float()


def run_decompose_reconstruct(name, batch, extra_ld, seed, mats=None, all_stages=True):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(seed)
    n = len(batch)
    mats = mats or [_gauss(s[0], s[1], gen) * (0.5 + i % 3) for i, s in enumerate(batch)]
    ar = Arena()
    descs, srcs, lds, wsp, wsb, views = [], [], [], [], [], {}
    for i, (s, mat) in enumerate(zip(batch, mats)):
        cores = [ar.output(shape, F32) for shape in T.core_shapes(s[2], s[3], s[4])]
        d = _desc(cores, s)
        src, ld = ar.pitched_input(mat, extra_ld)
        nb = int(lib.sow_tt_decompose_workspace_bytes(ctypes.byref(d)))
        assert nb > 0
        descs.append(d), srcs.append(src.data_ptr()), lds.append(ld), wsp.append(ar.workspace(nb)), wsb.append(nb)
        for k, c in enumerate(cores):
            views[f"c{i}.{k}"] = c
    arr = (_lib.TtDesc * n)(*descs)
    a_src, a_ld = (ctypes.c_void_p * n)(*srcs), (ctypes.c_int64 * n)(*lds)
    a_ws, a_wb = (ctypes.c_void_p * n)(*wsp), (ctypes.c_size_t * n)(*wsb)
    out = ar.run3(name + " decompose", lambda: _lib.check(lib.sow_tt_decompose_batch(arr, a_src, a_ld, n, a_ws, a_wb, SE._s()),
                                                          "sow_tt_decompose_batch"), views)
    # reconstruct the kernel's own cores (inputs now, NaN around them)
    ar2 = Arena()
    descs2, outs, lds2, views2 = [], [], [], {}
    for i, s in enumerate(batch):
        cin = [ar2.input(out[f"c{i}.{k}"]) for k in range(len(s[3]))]
        o, ld = ar2.pitched_output(s[0], s[1], extra_ld)
        descs2.append(_desc(cin, s)), outs.append(o.data_ptr()), lds2.append(ld)
        views2[f"m{i}"] = o
    arr2 = (_lib.TtDesc * n)(*descs2)
    a_out, a_ld2 = (ctypes.c_void_p * n)(*outs), (ctypes.c_int64 * n)(*lds2)
    rec = ar2.run3(name + " reconstruct", lambda: _lib.check(lib.sow_tt_reconstruct_batch(arr2, a_out, a_ld2, n, SE._s()),
                                                            "sow_tt_reconstruct_batch"), views2)
    total = {}
    for i, (s, mat) in enumerate(zip(batch, mats)):
        rows, cols, ranks, ind, outd = s
        cores = [out[f"c{i}.{k}"] for k in range(len(ind))]
        L0 = T.pad_interleave_ref(mat, ind, outd)
        st = T.check_tt_decomposition(cores, L0, ranks, ind, outd, name=f"{name}[{i}]")
        if "lapack" in st and all_stages:    # the fixed Gaussian cases: seeds chosen so that every stage is well conditioned
            assert st["lapack"]["counted"] == st["lapack"]["stages"], (name, i, st["lapack"])
        st["matrix"] = T.check_tt_matrix(rec[f"m{i}"], cores, ind, outd, rows, cols, name=f"{name}[{i}].to_matrix")
        stages = T.stage_shapes(ranks, ind, outd)
        if len(stages) == 1 and stages[0][3] == stages[0][0]:
            # r_1 = m: nothing is truncated, reconstruct(decompose(mat)) returns mat.  L_0 - Q R = (I - Q Q^T) L_0 + Q (Q^T L_0
            # - R): |I - Q Q^T| <= the orthonormality bound per element (times the column's 1-norm), and |Q^T L_0 - R| is
            # the projection check's noise, through |Q|.
            m, nc, kc, r = stages[0]
            Q = to64(cores[0]).reshape(m, r)
            L = L0.reshape(m, nc)
            lim = T.orth_bound(m, kc) * L.abs().sum(0, keepdim=True) + Q.abs() @ st["proj"]["noise"].reshape(r, nc) \
                + Q.abs() @ ulp(to64(cores[1]).reshape(r, nc), F32)
            extra = T.deinterleave(lim.reshape(-1), ind, outd)[:rows, :cols]
            ref, noise = to64(mat), T.tt_noise(cores, ind, outd, rows, cols)
            st["roundtrip"] = check_bound(rec[f"m{i}"], ref, ulp(ref, F32) + noise + extra, name=f"{name}[{i}].roundtrip")
        st["proj"].pop("noise", None)
        _fold(total, st)
    _note(name, total)
    return out, rec


RD_CASES = {   # id -> (batch, extra ld)
    "order1_copy_path": ([S["o1"], S["o1_pad"]], 0),
    "order2_rank3_padded_37x5": ([S["o2_r3"]], 0),
    "order2_rank16_100x60_pitched": ([S["o2_r16"]], 3),
    "order2_768x3072_rrest_wide_m_not_x64": ([S["o2_big"]], 0),
    "order2_full_rank_roundtrip": ([S["o2_full"]], 3),
    "order3_rank8_exact_512x512_both_rrest": ([S["o3_r8"]], 0),
    "order3_rank16_inner_bond_in_ne_out": ([S["o3_r16"]], 3),
    "order3_rank32_limit_512x1376": ([S["o3_r32"]], 0),
    "order3_rank9_8_one_wide_modes": ([S["o3_r9"]], 0),
    "order3_kc_lt_r_and_one_column_left": ([S["o3_kc"], S["o3_nc1"]], 3),
    "order3_rrest_rest_1": ([S["o3_rest1"]], 0),
    "order4_rrest_rest_1_m80_pitched": ([S["o4_rest1"], S["o3_rest1"]], 3),
    "order4_exact_81x81": ([S["o4_r4"]], 0),
    "order4_kc_lt_r_one_wide": ([S["o4_kc"]], 0),
    "order5": ([S["o5"]], 0),
    "order6": ([S["o6"]], 3),
    "batch16_mixed": ([S[k] for k in ("o1", "o2_r3", "o2_r16", "o3_r16", "o4_r4", "o5", "o3_kc", "o2_full")] * 2, 0),
    "batch17_mixed_second_chunk": (([S[k] for k in ("o2_r3", "o4_r4", "o1", "o3_r9", "o6", "o3_nc1", "o3_rest1")] * 3)[:17], 3),
    "batch33_mixed_third_chunk": (([S[k] for k in ("o2_r3", "o1_pad", "o4_kc", "o5", "o3_r16", "o2_r16", "o4_r4")] * 5)[:33], 0),
}


@pytest.mark.parametrize("case", list(RD_CASES), ids=list(RD_CASES))
def test_decompose_and_reconstruct_batch_against_fp64(case):
    batch, extra = RD_CASES[case]
    run_decompose_reconstruct(case, batch, extra, seed=len(case) + 17 * len(batch))


def check_low_rank_reproduced(name, cores, mat_ref, s, out=None, input_noise=None):
    """An order-2 train of rank r_1 over a matrix of TT rank 3 <= r_1 reproduces it: `out` (the kernel's reconstruction of
    `cores`; None: their float64 contraction) against mat_ref.  With L = L_0 [m, nc], Q = core 0, R = core 1:
      L - Q R = Q (Q^T L - R) + (L - Q Q^T L).
    The first term is the projection check's noise N through |Q|.  The second is zero in exact arithmetic.  In fp32 the
    three reflectors that span L's columns have the backward error b ||A_i|| per column of A = L[:, :3] (b = orth_bound),
    and a column L_j = A c_j + e_j carries it with ||c_j|| <= ||L_j|| / sigma_min(A), twice (the visible Q is within b of
    an orthogonal matrix): 2 b kappa_F(A) ||L_j||, kappa_F = ||A||_F / sigma_min(A); e_j, what the fp32 rounding of the
    matrix left outside rank 3, is at most (1 + kappa_F) sigma_4(L).  `out` adds one ulp and tt_noise."""
    rows, cols, ranks, ind, outd = s
    (m, nc, kc, r), = T.stage_shapes(ranks, ind, outd)
    L0 = T.pad_interleave_ref(mat_ref, ind, outd)
    st = T.check_tt_decomposition(cores, L0, ranks, ind, outd, input_noise=input_noise, name=name)
    Q, L = to64(cores[0]).reshape(m, r), L0.reshape(m, nc)
    A = L[:, :3]
    kap = float(A.norm() / torch.linalg.svdvals(A)[-1])
    sig4 = float(torch.linalg.svdvals(L)[3])
    lim = Q.abs() @ st["proj"]["noise"].reshape(r, nc) + 2 * T.orth_bound(m, kc) * kap * L.norm(dim=0, keepdim=True) + (1 + kap) * sig4
    if input_noise is not None:      # the panel factored the kernel's own L_0, input_noise away from this one
        lim = lim + to64(input_noise).reshape(m, nc)
    lim = T.deinterleave(lim.reshape(-1), ind, outd)[:rows, :cols]
    ref = to64(mat_ref)
    if out is None:
        out = T.tt_matrix_ref(cores, ind, outd, rows, cols)
    else:
        lim = lim + ulp(ref, F32) + T.tt_noise(cores, ind, outd, rows, cols)
    stats = {"low_rank": check_bound(out, ref, lim, name=f"{name}: the train against the matrix it stands for")}
    _note(name, stats)


def test_low_tt_rank_matrix_is_reproduced_by_a_rank16_train():
    """A sum of three Kronecker products has TT rank 3: the unfolding is exactly rank deficient (kappa = inf, no stage is
    compared with LAPACK), and the rank-16 train must return the matrix: through decompose + reconstruct, and as the
    first moment of a TTAdam step without state whose gradient is that matrix."""
    gen = torch.Generator().manual_seed(23)
    mat = _low_rank_kron(gen)
    s = spec(64, 64, [1, 16, 1])
    out, rec = run_decompose_reconstruct("kron3_rank16", [s], 0, seed=1, mats=[mat], all_stages=False)
    check_low_rank_reproduced("kron3_rank16 decompose + reconstruct", [out["c0.0"], out["c0.1"]], mat, s, out=rec["m0"])
    betas = (0.9, 0.999)
    inp = adam_item_inputs(s, 0, betas, 0.0, gen)
    inp["g"] = (mat.double() * 1e-2).float()
    res = run_ttadam("kron3_rank16 ttadam", [inp], betas, 0)
    refs, mags, *_ = T.ttadam_batch_ref(inp)
    check_low_rank_reproduced("kron3_rank16 ttadam m", [res["m0.0"], res["m0.1"]], refs["m"], s,
                              input_noise=T.pad_interleave_ref(T.C_M * U32 * mags["m"], s[3], s[4]))


@pytest.mark.parametrize("bad", ["rank33", "order7"])
def test_unsupported_trains_are_refused_and_touch_nothing(bad):
    lib = _lib.load()
    s = spec(64, 64, [1, 33, 1]) if bad == "rank33" else spec(128, 128, [1] + [2] * 6 + [1], [2] * 7, [2] * 7)
    ar = Arena()
    cores = [ar.output(shape, F32) for shape in T.core_shapes(s[2], s[3], s[4])][:_lib.TT_MAX_ORDER]
    d = _desc(cores, s)
    if bad == "order7":
        d.order = 7
    mat = ar.input(torch.randn(s[0], s[1]))
    outm = ar.output((s[0], s[1]), F32)
    ws = ar.workspace(1 << 16)
    arr = (_lib.TtDesc * 1)(d)
    one = lambda v: (ctypes.c_void_p * 1)(v)
    ld = (ctypes.c_int64 * 1)(s[1])
    assert lib.sow_tt_decompose_workspace_bytes(ctypes.byref(d)) == 0 and lib.sow_ttadam_workspace_bytes(ctypes.byref(d)) == 0
    ar.fill(0xFF)
    before = [SE._bits(v).clone() for _, _, _, v, _ in ar.outs]
    assert lib.sow_tt_decompose_batch(arr, one(mat.data_ptr()), ld, 1, one(ws), (ctypes.c_size_t * 1)(1 << 16), SE._s()) \
        == _lib.ERR_UNSUPPORTED
    assert lib.sow_tt_reconstruct_batch(arr, one(outm.data_ptr()), ld, 1, SE._s()) == _lib.ERR_UNSUPPORTED
    it = _lib.TtAdamItem()
    it.m, it.v = d, d
    it.param, it.grad, it.ld_param, it.ld_grad = outm.data_ptr(), mat.data_ptr(), s[1], s[1]
    it.step_size, it.lr_times_wd, it.has_state, it.workspace, it.workspace_bytes = 1e-3, 0.0, 0, ws, 1 << 16
    assert lib.sow_ttadam_batch((_lib.TtAdamItem * 1)(it), 1, 0.9, 0.999, 1e-8, SE._s()) == _lib.ERR_UNSUPPORTED
    ar.check_guards(bad)
    for b, (_, _, _, v, _) in zip(before, ar.outs):
        assert torch.equal(b, SE._bits(v)), f"{bad}: a refused call wrote to an output"


# ---- sow_ttadam_batch ----------------------------------------------------------------------------------------------------
def adam_item_inputs(s, has_state, betas, lr_wd, gen, v_kind="v", step=3, small_grad=True):
    rows, cols, ranks, ind, outd = s
    inp = dict(p0=T.small_and_plain_param(rows, cols, gen), g=T.quartered_grad(rows, cols, gen, small=small_grad and v_kind != "v_sq"),
               ranks=ranks, in_dims=ind, out_dims=outd, has_state=has_state, betas=betas, eps=1e-8, lr_wd=_f(lr_wd),
               step_size=_f(1e-3 * math.sqrt(1 - betas[1] ** step) / (1 - betas[0] ** step)), cores_m0=None, cores_v0=None)
    if has_state:
        inp["cores_m0"] = T.state_cores("m", rows, cols, ranks, ind, outd, gen)
        inp["cores_v0"] = T.state_cores(v_kind, rows, cols, ranks, ind, outd, gen)
    return inp


def _assert_decided(name, undecided, numel):
    """The cap of tt_numerics.MAX_UNDECIDED over the elements of a whole case."""
    assert undecided <= T.MAX_UNDECIDED * numel, \
        f"{name}: {undecided} of {numel} elements of p are undecided (reference interval wider than 2^-10 of the update)"


def run_ttadam(name, inputs, betas, extra_ld):
    lib = _lib.load()
    n = len(inputs)
    ar = Arena()
    items, views = [], {}
    for i, inp in enumerate(inputs):
        rows, cols = inp["p0"].shape
        s = (rows, cols, inp["ranks"], inp["in_dims"], inp["out_dims"])
        shapes = T.core_shapes(inp["ranks"], inp["in_dims"], inp["out_dims"])
        cm = [ar.output(sh, F32, initial=inp["cores_m0"][k].reshape(sh) if inp["has_state"] else None) for k, sh in enumerate(shapes)]
        cv = [ar.output(sh, F32, initial=inp["cores_v0"][k].reshape(sh) if inp["has_state"] else None) for k, sh in enumerate(shapes)]
        p, ldp = ar.pitched_output(rows, cols, extra_ld, initial=inp["p0"])
        g, ldg = ar.pitched_input(inp["g"], extra_ld)
        it = _lib.TtAdamItem()
        it.m, it.v = _desc(cm, s), _desc(cv, s)
        nb = int(lib.sow_ttadam_workspace_bytes(ctypes.byref(it.m)))
        it.param, it.grad, it.ld_param, it.ld_grad = p.data_ptr(), g.data_ptr(), ldp, ldg
        it.step_size, it.lr_times_wd, it.has_state = inp["step_size"], inp["lr_wd"], inp["has_state"]
        it.workspace, it.workspace_bytes = ar.workspace(nb), nb
        items.append(it)
        views[f"p{i}"] = p
        for k in range(len(shapes)):
            views[f"m{i}.{k}"], views[f"v{i}.{k}"] = cm[k], cv[k]
    arr = (_lib.TtAdamItem * n)(*items)
    out = ar.run3(name, lambda: _lib.check(lib.sow_ttadam_batch(arr, n, betas[0], betas[1], 1e-8, SE._s()), "sow_ttadam_batch"),
                  views)
    total, errors, undecided = {}, [], 0
    for i, inp in enumerate(inputs):
        d = len(inp["in_dims"])
        try:
            st = T.check_ttadam_batch(out[f"p{i}"], [out[f"m{i}.{k}"] for k in range(d)], [out[f"v{i}.{k}"] for k in range(d)],
                                      inp, name=f"{name}[{i} state={inp['has_state']}]", max_undecided=None)
        except NumericsError as e:       # report every item before failing: the first may not be the telling one
            errors.append(str(e))
            continue
        undecided += st["p"]["undecided_count"]
        for s_ in st.values():
            s_.pop("noise", None)
        _fold(total, st)
    _note(name, total)
    assert not errors, "\n".join(errors)
    _assert_decided(name, undecided, sum(inp["p0"].numel() for inp in inputs))
    return out


ADAM_CASES = {   # id -> (item specs with (shape key, has_state, v kind), betas, lr_wd, extra ld)
    "1_item_order3_rank8_state_b999_wd": ([("o3_r8", 1, "v_sq")], (0.9, 0.999), 1e-5, 0),
    "1_item_no_state_b999": ([("o2_r16", 0, "v")], (0.9, 0.999), 0.0, 0),
    "8_items_mixed_state_b999_pitched": ([("o2_r16", 0, "v"), ("o4_r4", 1, "v"), ("o1", 1, "v"), ("o3_r16", 1, "v"), ("o2_r3", 0, "v"),
                                          ("o3_kc", 1, "v"), ("o5", 0, "v"), ("o3_r9", 1, "v")], (0.9, 0.999), 1e-5, 3),
    "9_items_second_chunk_b95": ([("o4_r4", 1, "v"), ("o2_r3", 1, "v"), ("o1_pad", 0, "v"), ("o4_kc", 1, "v"), ("o6", 0, "v"),
                                  ("o2_full", 1, "v"), ("o3_nc1", 0, "v"), ("o5", 1, "v"), ("o3_r16", 0, "v")], (0.9, 0.95), 0.0, 0),
    "17_items_third_chunk_b999_wd": (([("o2_r3", 0, "v"), ("o4_r4", 1, "v"), ("o1", 0, "v"), ("o3_r9", 1, "v"), ("o5", 1, "v"),
                                       ("o3_nc1", 1, "v"), ("o4_rest1", 1, "v")] * 3)[:17], (0.9, 0.999), 1e-5, 3),
    "rank32_512x1376_state_b999": ([("o3_r32", 1, "v")], (0.9, 0.999), 1e-5, 0),
    "768x3072_rank16_no_state_b999": ([("o2_big", 0, "v")], (0.9, 0.999), 0.0, 0),
}
@pytest.mark.parametrize("case", list(ADAM_CASES), ids=list(ADAM_CASES))
def test_ttadam_batch_against_fp64(case):
    """Every case has small-parameter elements and betas whose fp32 difference 1.f - beta is inexact: a kernel that forms
    1 - beta in fp32 errs by 115 u of the update in p (beta2 = 0.999), against the 14 u term, and fails here."""
    items, betas, lr_wd, extra = ADAM_CASES[case]
    gen = torch.Generator().manual_seed(1000 + len(case))
    inputs = [adam_item_inputs(S[k], has, betas, lr_wd, gen, v_kind=vk) for k, has, vk in items]
    run_ttadam(case, inputs, betas, extra)


# ---- seeded sweep ----------------------------------------------------------------------------------------------------------
SWEEP_SEED, SWEEP_CASES = 20240611, 40
SWEEP_ELEMENTS = 1 << 22     # padded elements per case, all trains together: the float64 references stay in seconds


def _draw_spec(rng, budget, max_rank):
    """Order 1 - 6, modes of 2 - 12 (order 1: up to 40, so that its single core is more than a few elements), at most
    `budget` padded elements (the largest mode shrinks until the train fits), ranks up to max_rank within r_{k+1} <= r_k i_k
    o_k, and in 60 % of the draws fewer rows / columns than the modes hold."""
    order = rng.choice([1, 2, 2, 3, 3, 3, 4, 4, 5, 6])
    hi = 40 if order == 1 else 12
    dims = [rng.randint(2, hi) for _ in range(2 * order)]
    while math.prod(dims) > budget:
        dims[dims.index(max(dims))] -= 1
    ind, outd = dims[:order], dims[order:]
    ranks = [1]
    for k in range(order - 1):
        ranks.append(rng.randint(1, min(max_rank, ranks[k] * ind[k] * outd[k])))
    ranks.append(1)
    rows = rng.randint(math.prod(ind) // 2 + 1, math.prod(ind)) if rng.random() < 0.6 else math.prod(ind)
    cols = rng.randint(math.prod(outd) // 2 + 1, math.prod(outd)) if rng.random() < 0.6 else math.prod(outd)
    return (rows, cols, ranks, ind, outd)


def _sweep():
    """Half of the cases reconstruct + decompose, half TTAdam; a third of them keep every rank <= 8 (tt_eval<8>)."""
    rng = random.Random(SWEEP_SEED)
    cases = []
    for i in range(SWEEP_CASES):
        n = rng.choice([1, 2, 3, 5])
        max_rank = 8 if i % 3 == 1 else 32
        batch = [_draw_spec(rng, SWEEP_ELEMENTS // n, max_rank) for _ in range(n)]
        cases.append(("adam" if i % 2 else "rd", batch, rng.choice([0, 3]), rng.choice([(0.9, 0.999), (0.9, 0.95)]), i))
    return cases


SWEEP = _sweep()


def _sid(c):
    return f"{c[0]}{c[4]}_" + "+".join("x".join(f"{i}.{o}" for i, o in zip(s[3], s[4])) + "r" + "-".join(map(str, s[2][1:-1]))
                                       for s in c[1])


@pytest.mark.parametrize("case", SWEEP, ids=_sid)
def test_sweep_against_fp64(case):
    kind, batch, extra, betas, i = case
    if kind == "rd":
        run_decompose_reconstruct(_sid(case), batch, extra, seed=SWEEP_SEED + i, all_stages=False)   # drawn: counts printed
    else:
        gen = torch.Generator().manual_seed(SWEEP_SEED + i)
        # plain and large gradients only: where g vanishes p rests on the old m alone, and a drawn train of order 4 - 6 with
        # ranks above 20 evaluates m with a noise (sum r_k u of the |cores| contraction) above 2^-10 of |m| at 2 - 6 % of its
        # elements -- undecided by construction.  The fixed cases keep the zero and tiny quarters.
        inputs = [adam_item_inputs(s, (i + j) % 2, betas, 1e-5 if j % 2 else 0.0, gen, small_grad=False)
                  for j, s in enumerate(batch)]
        run_ttadam(_sid(case), inputs, betas, extra)


# ---- TTAdam.step -----------------------------------------------------------------------------------------------------------
def test_ttadam_step_batched_three_steps_against_fp64():
    """TTAdam.step (batched) on four parameters for three steps; before each step the kernel's own cores are copied out, so
    every step is checked on its own inputs and the lossy re-compression does not accumulate into the limit."""
    import torch.nn as nn

    from sow_amd import TTAdam
    assert TTAdam.batched
    ranks = [1, 8, 8, 1]
    shapes = [(512, 512), (100, 60), (81, 81), (200, 333)]
    gen = torch.Generator().manual_seed(77)
    ps = [nn.Parameter(T.small_and_plain_param(r, c, gen).to(DEV)) for r, c in shapes]
    lr, wd, betas = 1e-3, 0.01, (0.9, 0.999)
    opt = TTAdam([{"params": ps, "ranks": ranks}], lr=lr, weight_decay=wd, betas=betas)
    for step in range(1, 4):
        inputs = []
        for p, (r, c) in zip(ps, shapes):
            p.grad = (torch.randn(r, c, generator=gen, dtype=torch.float64) * 1e-2).float().to(DEV)
            ind, outd = T.default_dims(r, c, 3)
            st = opt.state[p]
            has = "exp_avg" in st
            inputs.append(dict(p0=p.data.cpu().clone(), g=p.grad.cpu(), ranks=ranks, in_dims=ind, out_dims=outd, has_state=int(has),
                               betas=betas, eps=1e-8, lr_wd=_f(lr * wd),
                               step_size=_f(lr * math.sqrt(1.0 - betas[1] ** step) / (1.0 - betas[0] ** step)),
                               cores_m0=[x.cpu().clone() for x in st["exp_avg"].cores] if has else None,
                               cores_v0=[x.cpu().clone() for x in st["exp_avg_sq"].cores] if has else None))
        opt.step()
        torch.cuda.synchronize()
        total, undecided = {}, 0
        for p, inp in zip(ps, inputs):
            st = opt.state[p]
            res = T.check_ttadam_batch(p.data.cpu(), [x.cpu() for x in st["exp_avg"].cores], [x.cpu() for x in st["exp_avg_sq"].cores],
                                       inp, name=f"TTAdam.step {step} {tuple(p.shape)}", max_undecided=None)
            undecided += res["p"]["undecided_count"]
            for s_ in res.values():
                s_.pop("noise", None)
            _fold(total, res)
        _note(f"TTAdam.step {step}", total)
        _assert_decided(f"TTAdam.step {step}", undecided, sum(p.numel() for p in ps))


# ---- coverage ----------------------------------------------------------------------------------------------------------------
def test_zz_tt_coverage():
    """Worst err / limit per check kind over the cases that ran, how many decomposition stages were compared with LAPACK,
    and every edge family reached by at least three cases.  Reachability is decided from the cases' own shapes: the tt_eval
    template from the largest rank of each launch chunk (16 trains, 8 items), and tt_eval counted only where it runs (every
    reconstructed train; TTAdam items with state)."""
    for k, (w, case) in sorted(WORST.items()):
        print(f"check {k:12s} worst err/limit {w:.3f}  ({case})")
    print(f"decomposition stages compared with LAPACK: {LAPACK_STAGES[0]} of {LAPACK_STAGES[1]}")
    reached = [features(b, 16) for b, _ in RD_CASES.values()]
    reached += [features([S[k] for k, _, _ in c[0]], 8, [has for _, has, _ in c[0]]) for c in ADAM_CASES.values()]
    for kind, batch, _, _, i in SWEEP:
        reached.append(features(batch, 16) if kind == "rd" else features(batch, 8, [(i + j) % 2 for j in range(len(batch))]))
    seen = {}
    for fs in reached:
        for f in fs:
            seen[f] = seen.get(f, 0) + 1
    print("cases per family:", dict(sorted(seen.items())))
    need = ["eval8", "eval32_inner", "rrest_wide", "rrest_wave", "rest=1", "kc<r", "order1", "mixed_order"]
    short = {f: seen.get(f, 0) for f in need if seen.get(f, 0) < 3}
    assert not short, f"families reached by fewer than 3 cases: {short}"
    assert all(w <= 1.0 for w, _ in WORST.values())
