"""The checks of tests/tt_numerics.py, tested on the CPU (no `gpu` mark), in the pattern of test_step_numerics_cpu.py.

The six kernels of sow_amd/csrc/tt_batch.hip are emulated in float32 in their own operation order: tt_eval's sequential
fmas over the bond, the Adam update of tt_adam_eval_kernel, the pad + interleave, the panel by fp32 LAPACK
(torch.linalg.qr), copy-out of Q and of R's triangle, and R[:, kc:] = Q^T L by sequential fmas (rest >= 512) or by 64 lane
sums and a shuffle tree (rest < 512).  The emulation has to pass every check with worst err / limit <= 0.7.  A fault
catalogue has to be rejected, and each fault records whether the max-norm `rel_err < 1e-4` of test_gpu_round3.py would have
passed it.
"""
import ctypes
import os

import pytest
import torch

import tt_numerics as T
from conftest import rel_err
from numerics import NumericsError

MARGIN = 0.7
F32 = torch.float32


def _f(x):
    return torch.tensor(x, dtype=torch.float64).float()


def fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64, the sum rounds once more before the fp32 rounding (a
    double rounding in 2^-29 of the cases, far below anything checked here)."""
    return (a.double() * b.double() + c.double()).float()


# ---- emulations --------------------------------------------------------------------------------------------------------
def tt_eval_emulate(cores, ranks, in_dims, out_dims, drop_rank_at=None):
    """tt_eval at every index of the padded tensor, interleaved order (flat fp32)."""
    cs = [c.float().reshape(s) for c, s in zip(cores, T.core_shapes(ranks, in_dims, out_dims))]
    vec = cs[0].reshape(-1, ranks[1])
    for k in range(1, len(cs)):
        rk, io, rn = ranks[k], in_dims[k] * out_dims[k], ranks[k + 1]
        ck = cs[k].reshape(rk, io, rn)
        nxt = torch.zeros(vec.shape[0], io, rn, dtype=F32)
        for a in range(rk):
            nxt = fma(vec[:, a, None, None], ck[a][None], nxt)
        if drop_rank_at == k:                      # fault: `b < rn - 1`
            nxt[..., rn - 1] = 0.0
        vec = nxt.reshape(-1, rn)
    return vec.reshape(-1)


def reconstruct_emulate(cores, ranks, in_dims, out_dims, rows, cols, fault=None):
    drop = None
    if fault == "drop_rank":
        drop = max(k for k in range(1, len(in_dims)) if ranks[k + 1] > 1)
    full = T.deinterleave(tt_eval_emulate(cores, ranks, in_dims, out_dims, drop), in_dims, out_dims)
    out = full[:rows, :cols].clone()
    if fault == "last_row_lost":                   # `rows - 1`: the last row keeps what the (zeroed) buffer held
        out[-1] = 0.0
    if fault == "last_col_lost":
        out[:, -1] = 0.0
    return out


def pad_interleave_emulate(mat, in_dims, out_dims, fault=None):
    L0 = T.pad_interleave_ref(mat, in_dims, out_dims).float()
    d = len(in_dims)
    if fault == "pad_wrap":                        # padding filled from the wrapped index instead of 0
        rows, cols = mat.shape
        ri = torch.arange(T._prod(in_dims)) % rows
        ci = torch.arange(T._prod(out_dims)) % cols
        L0 = T.pad_interleave_ref(mat[ri][:, ci], in_dims, out_dims).float()
    if fault == "interleave_swap":                 # (i_k, o_k) decoded in the other order at one level with i_k != o_k
        k = max(k for k in range(d) if in_dims[k] != out_dims[k])
        shape = [x for j in range(d) for x in (in_dims[j], out_dims[j])]
        full = L0.reshape(shape)
        L0 = full.transpose(2 * k, 2 * k + 1).contiguous().reshape(-1)
    return L0


def rrest_emulate(Q, L, kc, fault=None):
    """R[:, kc:] = Q^T L[:, kc:] as tt_stage_rrest_kernel sums it."""
    m, nc = L.shape
    rest = nc - kc
    r = Q.shape[1]
    if rest <= 0:
        return torch.zeros(r, 0, dtype=F32)
    mm = m - 1 if fault == "tail_m_minus_1" else m
    Lr = L[:, kc:]
    if rest >= 512:
        acc = torch.zeros(r, rest, dtype=F32)
        for i in range(mm):
            acc = fma(Q[i, :, None], Lr[i][None, :], acc)
        return acc
    steps = -(-mm // 64)
    Qp, Lp = torch.zeros(steps * 64, r, dtype=F32), torch.zeros(steps * 64, rest, dtype=F32)
    Qp[:mm], Lp[:mm] = Q[:mm], Lr[:mm]            # lanes past m add nothing (an fma with a zero product is exact)
    acc = torch.zeros(64, r, rest, dtype=F32)
    for t in range(steps):
        acc = fma(Qp[t * 64:(t + 1) * 64, :, None], Lp[t * 64:(t + 1) * 64, None, :], acc)
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        if fault == "shuffle_step_missing" and off == 1:
            continue
        acc = acc + acc[lanes ^ off]
    return acc[0]


def decompose_emulate(L0, ranks, in_dims, out_dims, fault=None):
    """decompose_stages on an fp32 L_0 (flat): fp32 cores."""
    rest = L0.float().reshape(-1)
    d = len(in_dims)
    cores = []
    shapes = T.stage_shapes(ranks, in_dims, out_dims)
    qt_buf = torch.zeros(max([m * r for m, _, _, r in shapes] + [1]), dtype=F32)
    for k, (m, nc, kc, r) in enumerate(shapes):
        L = rest.reshape(m, nc)
        Q, R = torch.linalg.qr(L[:, :kc].contiguous(), mode="complete" if r > kc else "reduced")
        Q = Q[:, :r].contiguous()
        Rn = torch.zeros(r, nc, dtype=F32)
        Rn[:kc, :kc] = torch.triu(R[:kc, :kc])
        if fault == "sign_flip" and k == len(shapes) - 1:     # one reflector's sign: Q column and R row negated together
            j = min(1, r - 1)
            Q[:, j] = -Q[:, j]
            Rn[j] = -Rn[j]
        Rn[:, kc:] = rrest_emulate(Q, L, kc, fault)
        if fault == "stale_qt" and k >= 1:
            core = qt_buf[:r * m].reshape(r, m).t().contiguous()   # stage k - 1's Q^T, read with this stage's strides
        else:
            core = Q
        qt_buf.zero_()
        qt_buf[:r * m] = Q.t().contiguous().reshape(-1)
        cores.append(core.reshape(ranks[k], in_dims[k], out_dims[k], r).clone())
        rest = Rn.reshape(-1)
    cores.append(rest.reshape(ranks[d - 1], in_dims[-1], out_dims[-1], 1).clone())
    return cores


def adam_emulate(inp, fault=None):
    """tt_adam_eval_kernel + decompose_stages of one item: p, new m cores, new v cores."""
    ranks, ind, outd = inp["ranks"], inp["in_dims"], inp["out_dims"]
    rows, cols = inp["p0"].shape
    b1, b2 = inp["betas"]
    b1f, b2f = _f(b1), _f(b2)
    c1, c2 = (1.0 - b1f, 1.0 - b2f) if fault == "one_minus_beta_fp32" else (_f(1.0 - b1), _f(1.0 - b2))
    P, G = inp["p0"].float(), inp["g"].float()
    if inp["has_state"]:
        M = T.deinterleave(tt_eval_emulate(inp["cores_m0"], ranks, ind, outd), ind, outd)[:rows, :cols]
        V = T.deinterleave(tt_eval_emulate(inp["cores_v0"], ranks, ind, outd), ind, outd)[:rows, :cols]
        if fault not in ("no_clamp", "clamp_after"):
            V = V.clamp(min=0.0)
    else:
        M, V = torch.zeros_like(P), torch.zeros_like(P)
    M = M * b1f + G * c1
    V = V * b2f + G * G * c2
    if fault == "clamp_after":
        V = V.clamp(min=0.0)
    Pn = P + (M / (torch.sqrt(V) + _f(inp["eps"]))) * (-_f(inp["step_size"]))
    if inp["lr_wd"] > 0:
        Pn = Pn + (P if fault == "wd_pre_update" else Pn) * (-_f(inp["lr_wd"]))
    pf = fault if fault in ("pad_wrap", "interleave_swap") else None
    cm = decompose_emulate(pad_interleave_emulate(M, ind, outd, pf), ranks, ind, outd, fault)
    cv = decompose_emulate(pad_interleave_emulate(V, ind, outd, pf), ranks, ind, outd, fault)
    return Pn, cm, cv


# ---- cases ---------------------------------------------------------------------------------------------------------------
# (rows, cols, ranks, in_dims, out_dims): orders 1 - 5, ranks <= 8 and > 8, padded and exact, in != out, a 1-wide mode,
# kc < r (the 30 x 20 and 20 x 12 cases), both R-tail branches (512 x 512: rest = 4096 and 56; 81 x 81: 729, 77, 5)
CASES = [
    (37, 5, [1, 1], [37], [5]),
    (37, 5, [1, 3, 1], [7, 7], [3, 3]),
    (100, 60, [1, 16, 1], [10, 10], [8, 8]),
    (81, 81, [1, 4, 4, 4, 1], [3] * 4, [3] * 4),
    (512, 512, [1, 8, 8, 1], [8] * 3, [8] * 3),
    (200, 90, [1, 16, 16, 1], [6, 6, 6], [5, 5, 4]),
    (60, 50, [1, 9, 8, 1], [4, 1, 16], [5, 11, 1]),
    (30, 20, [1, 32, 32, 1], [8, 2, 2], [6, 2, 2]),
    (20, 12, [1, 6, 12, 12, 1], [5, 2, 2, 1], [3, 2, 1, 2]),
    (30, 30, [1, 4, 8, 8, 4, 1], [2, 2, 2, 2, 2], [2, 2, 2, 2, 2]),
    (512, 1376, [1, 32, 32, 1], [8] * 3, [12] * 3),
]
IDS = ["%dx%d_r%s" % (c[0], c[1], "-".join(map(str, c[2]))) for c in CASES]
WORST = {}


def _note(label, stats):
    for k, s in stats.items():
        WORST[k] = max(WORST.get(k, 0.0), s["worst"])
    print(f"{label}: " + ", ".join(f"{k} {s['worst']:.3g}" + (f" [{s['counted']}/{s['stages']} stages]" if "counted" in s else "")
                                   for k, s in stats.items()))


def _gauss(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _margin(stats):
    for k, s in stats.items():
        assert s["worst"] <= MARGIN, (k, s["worst"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_decompose_and_reconstruct_emulation_passes_with_margin(case):
    rows, cols, ranks, ind, outd = case
    mat = _gauss(rows, cols, rows + cols)
    L0 = pad_interleave_emulate(mat, ind, outd)
    cores = decompose_emulate(L0, ranks, ind, outd)
    st = T.check_tt_decomposition(cores, T.pad_interleave_ref(mat, ind, outd), ranks, ind, outd, name=IDS[CASES.index(case)])
    if "lapack" in st:      # a Gaussian input: every stage is well enough conditioned to be compared with LAPACK
        assert st["lapack"]["counted"] == st["lapack"]["stages"], st["lapack"]
    out = reconstruct_emulate(cores, ranks, ind, outd, rows, cols)
    st["matrix"] = T.check_tt_matrix(out, cores, ind, outd, rows, cols)
    _note("decompose " + IDS[CASES.index(case)], st)
    _margin(st)
    # the references agree with each other: the float64 decomposition reproduces a full-rank train's input
    ref_cores = T.tt_decompose_ref(T.pad_interleave_ref(mat, ind, outd), ranks, ind, outd)
    if all(r == m for m, _, _, r in T.stage_shapes(ranks, ind, outd)):
        assert rel_err(T.tt_matrix_ref(ref_cores, ind, outd, rows, cols), mat) < 1e-12


def _adam_inputs(case, has_state, betas, lr_wd, seed, v_kind="v"):
    rows, cols, ranks, ind, outd = case
    gen = torch.Generator().manual_seed(seed)
    inp = dict(p0=T.small_and_plain_param(rows, cols, gen), g=T.quartered_grad(rows, cols, gen, small=v_kind != "v_sq"), ranks=ranks, in_dims=ind,
               out_dims=outd, has_state=has_state, betas=betas, eps=1e-8, lr_wd=float(_f(lr_wd)),
               step_size=float(_f(1e-3 * (1 - betas[1] ** 3) ** 0.5 / (1 - betas[0] ** 3))), cores_m0=None, cores_v0=None)
    if has_state:
        inp["cores_m0"] = T.state_cores("m", rows, cols, ranks, ind, outd, gen)
        inp["cores_v0"] = T.state_cores(v_kind, rows, cols, ranks, ind, outd, gen)
    return inp


ADAM = [(CASES[3], 1, (0.9, 0.999), 1e-5, "v"), (CASES[2], 0, (0.9, 0.999), 0.0, "v"), (CASES[4], 1, (0.9, 0.95), 0.0, "v_sq"),
        (CASES[5], 1, (0.9, 0.999), 1e-5, "v"), (CASES[0], 1, (0.9, 0.999), 1e-5, "v"), (CASES[7], 1, (0.9, 0.999), 0.0, "v"),
        (CASES[10], 1, (0.9, 0.999), 1e-5, "v")]


@pytest.mark.parametrize("case,has_state,betas,lr_wd,v_kind", ADAM, ids=lambda v: None)
def test_ttadam_emulation_passes_with_margin(case, has_state, betas, lr_wd, v_kind):
    inp = _adam_inputs(case, has_state, betas, lr_wd, seed=case[0] + has_state, v_kind=v_kind)
    # the reference data alone: the corner interval leaves at most 1 % of the elements undecided
    _, half, _, upd, _ = T.ttadam_p_interval(inp)
    share = T.undecided_share(half, upd)
    print(f"{case[:3]} state={has_state}: undecided {100 * share:.4f} %, median half-width / update "
          f"{float((half / upd.clamp_min(1e-300))[upd > 0].median()):.3g}")
    assert share <= T.MAX_UNDECIDED
    p, cm, cv = adam_emulate(inp)
    st = T.check_ttadam_batch(p, cm, cv, inp, name="ttadam")
    _note(f"ttadam {case[0]}x{case[1]} r{case[2]} state={has_state} betas={betas}", st)
    _margin(st)


# ---- fault catalogue -------------------------------------------------------------------------------------------------------
REL_ERR_ACCEPTS = {}


def _rel_err_passes(outs, refs):
    """Would `rel_err < 1e-4` of every output against its float64 reference have passed?"""
    return all(rel_err(o.reshape(-1), r.reshape(-1)) < 1e-4 for o, r in zip(outs, refs))


def _adam_refs(inp):
    refs, mags, *_ = T.ttadam_batch_ref(inp)
    dims = (inp["in_dims"], inp["out_dims"])
    return refs, [T.tt_decompose_ref(T.pad_interleave_ref(refs[k], *dims), inp["ranks"], *dims) for k in ("m", "v")]


def _reject_adam(fault, inp, where=None):
    p, cm, cv = adam_emulate(inp, fault)
    with pytest.raises(NumericsError) as e:
        T.check_ttadam_batch(p, cm, cv, inp, name=fault)
    if where:
        assert where in str(e.value), (fault, str(e.value))
    refs, (rm, rv) = _adam_refs(inp)
    ok = _rel_err_passes([p] + cm + cv, [refs["p"]] + rm + rv)
    REL_ERR_ACCEPTS[fault] = REL_ERR_ACCEPTS.get(fault, True) and ok
    print(f"fault {fault}: rejected ({str(e.value)[:110]} ...); rel_err < 1e-4 would have {'PASSED' if ok else 'failed'} it")


def test_fault_one_minus_beta_in_fp32():
    """1.f - 0.999f errs by 1.29e-5 = 216 u in the g^2 term of v.  Without state v is that term alone: rejected in the v
    cores (projection identity) and in p (sqrt halves it: 108 u against the 14 u term)."""
    inp = _adam_inputs(CASES[2], 0, (0.9, 0.999), 0.0, seed=3)
    p, cm, cv = adam_emulate(inp, "one_minus_beta_fp32")
    good_p, good_m, good_v = adam_emulate(inp)
    with pytest.raises(NumericsError) as e:      # p alone
        T.check_ttadam_batch(p, good_m, good_v, inp, name="fp32 1 - beta")
    assert ".p:" in str(e.value)
    print("p of the fp32 1 - beta, no state:", str(e.value)[:160])
    with pytest.raises(NumericsError) as e:      # the v cores alone
        T.check_ttadam_batch(good_p, good_m, cv, inp, name="fp32 1 - beta")
    assert ".v." in str(e.value)
    print("v cores of the fp32 1 - beta, no state:", str(e.value)[:160])
    _reject_adam("one_minus_beta_fp32", inp)
    # With state the fault shows only where (1 - b2) g^2 dominates v, the large-gradient quarter: where b2 v dominates, a
    # 1.3e-5 error of the g^2 term is below the reconstruction noise of v and no test can see it.
    inp = _adam_inputs(CASES[4], 1, (0.9, 0.999), 0.0, seed=4)
    p, cm, cv = adam_emulate(inp, "one_minus_beta_fp32")
    good_p, good_m, good_v = adam_emulate(inp)
    with pytest.raises(NumericsError):
        T.check_ttadam_batch(p, good_m, good_v, inp, name="with state")
    rows = inp["p0"].shape[0]
    mid, half, mag, _, _ = T.ttadam_p_interval(inp)
    over = (p.double() - mid).abs() > half + T.C_P * T.U32 * mag + T.ulp(mid, F32)
    assert over[3 * rows // 4:].any() and not over[:rows // 2].any(), "expected in the large-gradient quarter only"
    assert REL_ERR_ACCEPTS["one_minus_beta_fp32"], "the max-norm tolerance was expected to hide this fault"


@pytest.mark.parametrize("fault", ["no_clamp", "clamp_after"])
def test_fault_clamp(fault):
    inp = _adam_inputs(CASES[4], 1, (0.9, 0.95), 0.0, seed=5, v_kind="v_sq")
    v0 = T.tt_matrix_ref(inp["cores_v0"], inp["in_dims"], inp["out_dims"], *inp["p0"].shape)
    assert (v0 < 0).any()
    _reject_adam(fault, inp)


def test_fault_weight_decay_on_the_old_p():
    _reject_adam("wd_pre_update", _adam_inputs(CASES[3], 1, (0.9, 0.999), 1e-3, seed=6), where=".p")


def test_fault_padding_not_zero():
    _reject_adam("pad_wrap", _adam_inputs(CASES[2], 0, (0.9, 0.95), 0.0, seed=7))


def test_fault_interleave_swapped():
    _reject_adam("interleave_swap", _adam_inputs(CASES[5], 1, (0.9, 0.999), 0.0, seed=8))


def _reject_decompose(fault, case, seed=11):
    rows, cols, ranks, ind, outd = case
    mat = _gauss(rows, cols, seed)
    L0 = T.pad_interleave_ref(mat, ind, outd)
    cores = decompose_emulate(pad_interleave_emulate(mat, ind, outd, fault if fault in ("pad_wrap", "interleave_swap") else None),
                              ranks, ind, outd, fault)
    with pytest.raises(NumericsError) as e:
        T.check_tt_decomposition(cores, L0, ranks, ind, outd, name=fault)
    ok = _rel_err_passes(cores, T.tt_decompose_ref(L0, ranks, ind, outd))
    REL_ERR_ACCEPTS[fault + "/decompose"] = ok
    print(f"fault {fault}: rejected ({str(e.value)[:110]} ...); rel_err < 1e-4 would have {'PASSED' if ok else 'failed'} it")
    return str(e.value)


def test_fault_decompose_layout():
    _reject_decompose("pad_wrap", CASES[2])
    _reject_decompose("interleave_swap", CASES[5])


def test_fault_householder_sign():
    """Orthonormal and still a decomposition of the input: only the comparison with LAPACK sees it."""
    rows, cols, ranks, ind, outd = CASES[4]
    msg = _reject_decompose("sign_flip", CASES[4])
    assert "vs LAPACK" in msg
    mat = _gauss(rows, cols, 11)
    cores = decompose_emulate(pad_interleave_emulate(mat, ind, outd), ranks, ind, outd, "sign_flip")
    good = decompose_emulate(pad_interleave_emulate(mat, ind, outd), ranks, ind, outd)
    assert rel_err(T.tt_matrix_ref(cores, ind, outd, rows, cols), T.tt_matrix_ref(good, ind, outd, rows, cols)) < 1e-6


def test_fault_r_tail():
    _reject_decompose("tail_m_minus_1", CASES[4])            # both branches at 512 x 512
    _reject_decompose("shuffle_step_missing", CASES[4])
    _reject_decompose("tail_m_minus_1", CASES[2])            # rest < 512 only


def test_fault_stale_q():
    _reject_decompose("stale_qt", CASES[3])
    _reject_decompose("stale_qt", CASES[4])


@pytest.mark.parametrize("fault", ["drop_rank", "last_row_lost", "last_col_lost"])
def test_fault_reconstruct(fault):
    for case in (CASES[5], CASES[3]):
        rows, cols, ranks, ind, outd = case
        cores = [c.float() for c in T.tt_decompose_ref(T.pad_interleave_ref(_gauss(rows, cols, 12), ind, outd), ranks, ind, outd)]
        out = reconstruct_emulate(cores, ranks, ind, outd, rows, cols, fault)
        with pytest.raises(NumericsError):
            T.check_tt_matrix(out, cores, ind, outd, rows, cols, name=fault)
        ok = rel_err(out, T.tt_matrix_ref(cores, ind, outd, rows, cols)) < 1e-4
        REL_ERR_ACCEPTS[fault] = REL_ERR_ACCEPTS.get(fault, True) and ok
        print(f"fault {fault}: rejected; rel_err < 1e-4 would have {'PASSED' if ok else 'failed'} it")


def test_zz_report():
    print("emulation, worst err / limit per check:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    print("faults that rel_err < 1e-4 accepts:", sorted(k for k, v in REL_ERR_ACCEPTS.items() if v))
    assert all(v <= MARGIN for v in WORST.values())


def test_ttadam_workspace_is_two_decompose_workspaces():
    from sow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsow_amd.so is not built")
    lib = _lib.load()
    for rows, cols, ranks, ind, outd in CASES:
        d = _lib.TtDesc()
        d.order = len(ind)
        keep = [torch.zeros(1) for _ in ind]
        for k in range(len(ind)):
            d.cores[k], d.in_dims[k], d.out_dims[k] = keep[k].data_ptr(), ind[k], outd[k]
        for k, r in enumerate(ranks):
            d.ranks[k] = r
        d.rows, d.cols = rows, cols
        one = lib.sow_tt_decompose_workspace_bytes(ctypes.byref(d))
        assert one > 0 and lib.sow_ttadam_workspace_bytes(ctypes.byref(d)) == 2 * one
