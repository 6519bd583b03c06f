"""The comparators of tests/numerics.py, tested on the CPU (no `gpu` mark).

Each checked stage is emulated the way the kernels compute it: bf16 (or fp32) inputs, exact products, fp32 running sums
of 64-wide K or token blocks, and rounding to nearest even at the documented points -- h rounded to bf16 before the
second product, y rounded once, dh in bf16, the slab sums of the weight gradients in fp32 in a fixed order, and for fp32
the exact 3-plane bf16 split of chain3f.hip (split3_scalar) with its six plane products.  The emulation has to pass every
checker with margin (worst err / limit <= 0.7); every fault of the catalogue has to be rejected.  The catalogue also
records whether today's `rel_err` tolerance (2e-2 for bf16, 1e-5 for fp32) would have passed the fault: that is the gap
these checks close.
"""
import pytest
import torch

from conftest import rel_err
import fuzz_plan as FP
import test_gpu_elementwise as E
from numerics import (MAX_INEXACT, UNIT_ROUNDOFF, NumericsError, accumulation_term, bound, check_bound, check_gaps,
                      check_h_save, check_rounded, fp32_floor, gemm_epilogue, gemm_f32_bound, ref64, rne, ulp)

BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
U16 = UNIT_ROUNDOFF[BF16]
MARGIN = 0.7


# ---- emulation ------------------------------------------------------------------------------------------------------
def _data(shape, dtype, gen, std=1.0):
    """Random values exactly representable in `dtype`, held as float64."""
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * std).to(dtype).double()


def mm32(a, b, block=64):
    """a [M, K] . b [K, N] as the kernels sum it: exact products, each 64-wide K block summed, the blocks added one after
    the other into an fp32 accumulator (float64 out)."""
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], block):
        acc += (a[:, k0:k0 + block] @ b[k0:k0 + block]).float()
    return acc.double()


def split3(v):
    """chain3f.hip split3_scalar: fp32 value = hi + mid + lo, each a truncated bf16 (exact)."""
    v32 = v.float()
    hi = (v32.view(torch.int32) & ~0xFFFF).view(torch.float32)
    r = v32 - hi
    mid = (r.view(torch.int32) & ~0xFFFF).view(torch.float32)
    q = r - mid
    lo = (q.view(torch.int32) & ~0xFFFF).view(torch.float32)
    return [p.double() for p in (hi, mid, lo)]


def mm3f(a, b, odd_lo_fault=False):
    """fp32 a . b on the bf16 matrix pipe: the six plane products hi.hi + hi.mid + mid.hi + hi.lo + lo.hi + mid.mid (the
    dropped ones are below 2^-24 relative), fp32 sums of 64-wide K blocks.  odd_lo_fault: the lo plane of every odd K lane
    of `a` replaced by its even neighbour's (a lane mix-up of the kind DESIGN section 4 records for bit_cast)."""
    pa, pb = split3(a), split3(b)
    if odd_lo_fault:
        lo = pa[2].clone()
        lo[:, 1::2] = lo[:, 0::2][:, : lo[:, 1::2].shape[1]]
        pa[2] = lo
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], 64):
        s = sum(pa[i][:, k0:k0 + 64] @ pb[j][k0:k0 + 64] for i in range(3) for j in range(3) if i + j <= 2)
        acc += s.float()
    return acc.double()


def h_save_of(h_live, r):
    """[T, 64] h_save layout: live columns, zeros, 1.0 in column 63 when r <= 63."""
    h = torch.zeros(h_live.shape[0], 64, dtype=torch.float64)
    h[:, :r] = h_live
    if r <= 63:
        h[:, 63] = 1.0
    return h


def emulate_bf16(x, A, B, bias, dy, s, W=None, *, drop_last_token=False, drop_last_col=False, store="rne",
                 y_twice=False):
    """The bf16 layer as the fused kernels compute it (chain2 / gemm4h forward, chain2 backward, skinny-TN weight
    gradients), with optional faults.  Returns dict of outputs (float64 holding bf16 values) and h_save [T, 64]."""
    r = A.shape[1]
    rnd = rne_bf16 if store == "rne" else trunc_bf16
    xk = x.clone()
    if drop_last_col:
        xk[:, -1] = 0
    h = rne(mm32(x, A) * s, BF16)
    if W is not None:
        acc = mm32(xk, W)
        if y_twice:   # dense accumulator written first, then re-read with beta = 1 and rounded again
            acc = rne(acc, BF16)
        y = rnd((acc + mm32(h, B)).float().double() + bias)
    else:
        y = rnd((mm32(h, B) + bias).float().double())
    dh = rne(mm32(dy, B.t()) * s, BF16)
    dx = rne(mm32(dh, A.t()) + (mm32(dy, W.t()) if W is not None else 0), BF16)
    tok = slice(0, x.shape[0] - 1) if drop_last_token else slice(None)
    dA = rne(mm32(x[tok].t(), dh[tok]), BF16)
    dB = rne(mm32(h[tok].t(), dy[tok]), BF16)
    dbias = rne(mm32(torch.ones(1, dy[tok].shape[0], dtype=torch.float64), dy[tok]).flatten(), BF16)
    return dict(h_save=h_save_of(h, r), y=y, dx=dx, dA=dA, dB=dB, dbias=dbias, dh=dh)


def rne_bf16(v):
    return rne(v, BF16)


def trunc_bf16(v):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero)."""
    return (v.float().view(torch.int32) & ~0xFFFF).view(torch.float32).double()


def layer_refs(x, A, B, bias, dy, s, h, W=None):
    """float64 references of every stage from the kernel's own visible intermediate h (= h_save[:, :r]), and the bounds of
    the stages with a hidden bf16 dh and the fp32 noise floors of the others: (refs, bounds)."""
    acc = x @ W if W is not None else 0
    dh64 = s * dy @ B.t()
    refs = dict(h=ref64(lambda a, b: s * (a @ b), x, A),
                y=acc + h @ B + bias,
                dB=h.t() @ dy, dbias=dy.sum(0),
                dA=x.t() @ dh64, dx=dh64 @ A.t() + (dy @ W.t() if W is not None else 0))
    T, d_in = x.shape
    hh, dy2, xx = h * h, dy * dy, x * x
    floors = dict(h=fp32_floor(xx @ (A * A) * s * s, d_in),
                  y=fp32_floor(hh @ (B * B) + (xx @ (W * W) if W is not None else 0), d_in + 64),
                  dB=fp32_floor(hh.t() @ dy2, T), dbias=fp32_floor(dy2.sum(0), T))
    bounds = dict(dA=bound(refs["dA"], BF16, accumulation_term(xx.t() @ (dh64 * dh64), U16)),
                  dx=bound(refs["dx"], BF16, accumulation_term((dh64 * dh64) @ (A * A).t(), U16)),
                  **floors)
    return refs, bounds


def check_layer_bf16(out, refs, bounds, r):
    """Every stage checked; the stats of each."""
    st = dict(h=check_h_save(out["h_save"], refs["h"], r, BF16, acc=bounds["h"]),
              y=check_rounded(out["y"], refs["y"], BF16, acc=bounds["y"], name="y"),
              dB=check_rounded(out["dB"], refs["dB"], BF16, acc=bounds["dB"], name="dB"),
              dbias=check_rounded(out["dbias"], refs["dbias"], BF16, acc=bounds["dbias"], name="dbias"),
              dA=check_bound(out["dA"], refs["dA"], bounds["dA"], name="dA"),
              dx=check_bound(out["dx"], refs["dx"], bounds["dx"], name="dx"))
    return st


def _layer_inputs(T, d_in, d_out, r, seed, dense=False):
    g = torch.Generator().manual_seed(seed)
    x = _data((T, d_in), BF16, g)
    A = _data((d_in, r), BF16, g, 0.05)
    B = _data((r, d_out), BF16, g, 0.05)
    bias = _data((d_out,), BF16, g, 0.1)
    dy = _data((T, d_out), BF16, g)
    W = _data((d_in, d_out), BF16, g, 0.02) if dense else None
    return x, A, B, bias, dy, W


# ---- the comparators themselves --------------------------------------------------------------------------------------
def test_ulp_and_rne_match_the_formats():
    v = torch.tensor([1.0, 1.5, 3.0, -0.75, 1e-3, 0.0, 2.0 ** -130])
    assert ulp(v, BF16).tolist()[:4] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]
    assert ulp(v, F32).tolist()[:3] == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
    assert float(ulp(torch.tensor([0.0]), BF16)) == 2.0 ** (-126 - 7)
    # one-step RNE from float64 agrees with torch's own fp32 -> bf16 rounding wherever fp32 holds the value exactly
    g = torch.Generator().manual_seed(1)
    f = torch.randn(100000, generator=g) * 10
    assert torch.equal(rne(f.double(), BF16), f.bfloat16().double())
    # ties go to even: 1 + 2^-8 sits halfway between 1 and 1 + 2^-7
    assert float(rne(torch.tensor([1 + 2.0 ** -8], dtype=torch.float64), BF16)) == 1.0
    assert float(rne(torch.tensor([1 + 3 * 2.0 ** -8], dtype=torch.float64), BF16)) == 1 + 2 * 2.0 ** -7
    d = torch.randn(1000, generator=g, dtype=torch.float64)
    assert torch.equal(rne(d, F32), d.float().double())


def test_failure_report_names_element_ratio_count_and_tail():
    ref = torch.randn(200, 130, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    out = rne(ref, BF16)
    out[-1, 5] += 4 * float(ulp(out[-1, 5:6], BF16))
    with pytest.raises(NumericsError, match=r"worst element \(199, 5\).*1 of 26000 elements over the limit.*"
                                            r"1/1 in the last row block"):
        check_rounded(out, ref, BF16, name="y")
    out = ref.clone()
    out[:, -1] = float("nan")
    with pytest.raises(NumericsError, match="200 of 26000.*200/200 in the last column block"):
        check_bound(out, ref, torch.full_like(ref, 1e-3), name="dA")


@pytest.mark.parametrize("K", [512, 4096, 11008])
def test_single_rounding_inexact_fraction_is_small(K):
    """Calibration of MAX_INEXACT: an fp32-accumulated product rounded once differs from RNE(fp64) in a small fraction of
    the elements; truncation and double rounding in far more."""
    g = torch.Generator().manual_seed(K)
    a, b = _data((256, K), BF16, g), _data((K, 256), BF16, g, 0.02)
    c = _data((256, 256), BF16, g)
    ref = a @ b + c
    acc = (mm32(a, b) + c).float().double()
    st = check_rounded(rne(acc, BF16), ref, BF16, name="once")
    assert st["inexact"] <= MAX_INEXACT / 10, st
    trunc = trunc_bf16(acc)
    twice = rne((rne(mm32(a, b), BF16) + c).float().double(), BF16)
    frac = lambda o: float((o != rne(ref, BF16)).double().mean())   # noqa: E731
    assert frac(trunc) > 0.3 and frac(twice) > 0.1, (frac(trunc), frac(twice))
    print(f"K={K}: inexact once {100 * st['inexact']:.4f} %, truncated {100 * frac(trunc):.1f} %, "
          f"rounded twice {100 * frac(twice):.1f} %")


# ---- the emulated kernels pass every checker with margin --------------------------------------------------------------
@pytest.mark.parametrize("T,d_in,d_out,r,dense", [(8193, 256, 264, 50, False), (32769, 128, 72, 16, False),
                                                  (65, 1000, 264, 63, False), (4097, 512, 264, 64, True),
                                                  (1, 64, 8, 1, False)])
def test_bf16_emulation_passes_with_margin(T, d_in, d_out, r, dense):
    x, A, B, bias, dy, W = _layer_inputs(T, d_in, d_out, r, seed=T + r, dense=dense)
    s = 0.5
    out = emulate_bf16(x, A, B, bias, dy, s, W)
    refs, bounds = layer_refs(x, A, B, bias, dy, s, out["h_save"][:, :r], W)
    st = check_layer_bf16(out, refs, bounds, r)
    worst = {k: round(st[k]["worst"], 3) for k in ("dA", "dx")}
    inexact = {k: round(100 * st[k]["inexact"], 4) for k in ("h", "y", "dB", "dbias")}
    print(f"T={T} {d_in}->{d_out} r={r} dense={dense}: worst err/bound {worst}, inexact % {inexact}")
    assert max(worst.values()) <= MARGIN, worst
    assert max(st[k]["inexact"] for k in inexact) <= MAX_INEXACT / 10, inexact


def _f32_layer(T, d_in, d_out, r, seed, fault=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, d_in, generator=g).double()
    A = (torch.randn(d_in, r, generator=g) * 0.05).double()
    B = (torch.randn(r, d_out, generator=g) * 0.05).double()
    bias = (torch.randn(d_out, generator=g) * 0.1).double()
    s = 0.5
    h = (mm3f(x, A, odd_lo_fault=fault).float() * s).double()
    y = (mm3f(h, B).float() + bias.float()).double()
    ref_h = s * x @ A
    ref_y = ref_h @ B + bias
    u = UNIT_ROUNDOFF[F32]
    bh = bound(ref_h, F32, accumulation_term((x * x) @ (A * A) * s * s, u, d_in))
    by = bound(ref_y, F32, accumulation_term((x * x) @ (A * A) @ (B * B) * s * s, u, d_in + r))
    return (h, ref_h, bh), (y, ref_y, by)


def test_fp32_split_emulation_passes_with_margin():
    (h, rh, bh), (y, ry, by) = _f32_layer(2048, 512, 264, 50, seed=3)
    wh, wy = check_bound(h, rh, bh, name="h")["worst"], check_bound(y, ry, by, name="y")["worst"]
    print(f"fp32 3-plane split: worst ratio h {wh:.3f}, y {wy:.3f}")
    assert max(wh, wy) <= MARGIN


# ---- fault catalogue ------------------------------------------------------------------------------------------------
def _fault_drop_last_token(T, which):
    r = 16
    x, A, B, bias, dy, _ = _layer_inputs(T, 256, 264, r, seed=100 + T)
    good = emulate_bf16(x, A, B, bias, dy, 1.0)
    bad = emulate_bf16(x, A, B, bias, dy, 1.0, drop_last_token=True)
    refs, bounds = layer_refs(x, A, B, bias, dy, 1.0, good["h_save"][:, :r])
    if which == "dA":
        return bad["dA"], refs["dA"], lambda o: check_bound(o, refs["dA"], bounds["dA"], name="dA")
    return bad[which], refs[which], lambda o: check_rounded(o, refs[which], BF16, acc=bounds[which], name=which)


def _fault_drop_last_column_of_y():
    r = 16
    x, A, B, bias, dy, W = _layer_inputs(512, 1000, 264, r, seed=7, dense=True)
    bad = emulate_bf16(x, A, B, bias, dy, 1.0, W, drop_last_col=True)
    refs, bounds = layer_refs(x, A, B, bias, dy, 1.0, bad["h_save"][:, :r], W)
    return bad["y"], refs["y"], lambda o: check_rounded(o, refs["y"], BF16, acc=bounds["y"], name="y")


def _fault_y_store(kind):
    r = 16
    x, A, B, bias, dy, W = _layer_inputs(2048, 4096, 264, r, seed=8, dense=True)
    bad = emulate_bf16(x, A, B, bias, dy, 1.0, W, store="trunc" if kind == "trunc" else "rne", y_twice=kind == "twice")
    refs, bounds = layer_refs(x, A, B, bias, dy, 1.0, bad["h_save"][:, :r], W)
    return bad["y"], refs["y"], lambda o: check_rounded(o, refs["y"], BF16, acc=bounds["y"], name="y")


def _fault_f32_odd_lo_plane():
    (h, rh, bh), _ = _f32_layer(2048, 512, 264, 50, seed=3, fault=True)
    return h, rh, lambda o: check_bound(o, rh, bh, name="h")


def _fault_ones_column_at_r():
    r = 50
    x, A, B, bias, dy, _ = _layer_inputs(512, 256, 264, r, seed=9)
    good = emulate_bf16(x, A, B, bias, dy, 1.0)
    bad = good["h_save"].clone()
    bad[:, 63], bad[:, r] = 0.0, 1.0
    ref = x @ A
    # rel_err of the whole [T, 64] buffer against the contract's layout
    return bad, h_save_of(ref, r), lambda o: check_h_save(o, ref, r, BF16)


def _wide_bf16(T, d_in, d_out, r, seed, drop_from=None):
    """A wide (r > 64) bf16 layer's weight gradients as skinny_tn_wide.hip forms them -- h [T, r] (unscaled x A, saved),
    dh = RNE(s dY B^T), fp32 slab partials summed in slab order, one rounding -- with the tokens from `drop_from` on left
    out (a lost last slab).  Returns (dB, its reference, its check)."""
    g = torch.Generator().manual_seed(seed)
    x, A, B = _data((T, d_in), BF16, g), _data((d_in, r), BF16, g, 0.05), _data((r, d_out), BF16, g, 0.05)
    dy = _data((T, d_out), BF16, g)
    h = rne(mm32(x, A), BF16)
    _, ln = FP.tnw_pick_slabs(T, d_in, d_out)
    stop = T if drop_from is None else drop_from
    acc = torch.zeros(r, d_out, dtype=torch.float32)
    for t0 in range(0, stop, ln):
        t1 = min(t0 + ln, stop)
        acc += mm32(h[t0:t1].t(), dy[t0:t1], block=64).float()
    dB = rne(acc.double(), BF16)
    ref = h.t() @ dy
    return dB, ref, lambda o: check_rounded(o, ref, BF16, acc=fp32_floor((h * h).t() @ (dy * dy), T), name="dB")


def _fault_tnw_last_slab():
    T = next(t for t in range(8193, 12000) if t % FP.tnw_pick_slabs(t, 256, 264)[1] == 1)   # k * slab_len + 1
    ns, ln = FP.tnw_pick_slabs(T, 256, 264)   # the last slab holds one token
    assert T % ln == 1 and ns >= 2
    out, ref, chk = _wide_bf16(T, 256, 264, 96, seed=11, drop_from=(ns - 1) * ln)
    return out, ref, chk


def _fault_chain3f_last_column(odd=True):
    """fp32 forward at odd d_out (chain3f's predicated column tail): the last column keeps only the bias."""
    T, d_in, d_out, r = 256, 128, 131, 24
    g = torch.Generator().manual_seed(12)
    x = torch.randn(T, d_in, generator=g).double()
    A, B = (torch.randn(d_in, r, generator=g) * 0.05).double(), (torch.randn(r, d_out, generator=g) * 0.05).double()
    bias = (torch.randn(d_out, generator=g) * 0.1).double()
    h = (mm3f(x, A).float() * 0.5).double()
    y = (mm3f(h, B).float() + bias.float()).double()
    y[:, -1] = bias[-1].float().double()
    ref = h @ B + bias
    by = bound(ref, F32, accumulation_term((h * h) @ (B * B), UNIT_ROUNDOFF[F32], 64 + r))
    return y, ref, lambda o: check_bound(o, ref, by, name="y")


def _fault_gemm_spills_into_ldc_gap():
    """A strided C (ldc > N) whose store writes one element past every row: the values of the view are right, the gap
    guard (the GPU test's check_gaps over the whole buffer) rejects the store."""
    M, N, K, ldc, sentinel = 64, 100, 48, 104, E.SENTINEL
    g = torch.Generator().manual_seed(13)
    a, b = _data((M, K), BF16, g), _data((K, N), BF16, g, 0.05)
    ref = a @ b
    buf = torch.full((M * ldc + 2 * E.GUARD,), sentinel, dtype=torch.float64)
    live = torch.zeros(buf.numel(), dtype=torch.bool)
    live[E.GUARD:E.GUARD + M * ldc].view(M, ldc)[:, :N] = True
    rows = buf[E.GUARD:E.GUARD + M * ldc].view(M, ldc)
    rows[:, :N + 1] = torch.cat([rne(mm32(a, b), BF16), rne(mm32(a, b), BF16)[:, -1:]], dim=1)   # one element too many
    out = rows[:, :N].clone()

    def chk(o):
        check_rounded(o, ref, BF16, acc=fp32_floor((a * a) @ (b * b), K), name="C")
        check_gaps(buf, live, sentinel, name="C buffer")
    return out, ref, chk


def _fault_f16_y_truncated():
    """f16 y stored by dropping the low 13 bits of the fp32 sum instead of rounding to nearest even."""
    g = torch.Generator().manual_seed(14)
    T, d_in, d_out, r = 2048, 512, 264, 32
    x, A, B = _data((T, d_in), F16, g), _data((d_in, r), F16, g, 0.05), _data((r, d_out), F16, g, 0.05)
    bias = _data((d_out,), F16, g, 0.1)
    h = rne(mm32(x, A), F16)
    acc = (mm32(h, B) + bias).float()
    y = (acc.view(torch.int32) & ~0x1FFF).view(torch.float32).to(F16).double()   # exact: the low 13 bits are gone
    ref = h @ B + bias
    return y, ref, lambda o: E._rounded(o, ref, F16, fp32_floor((h * h) @ (B * B), 64), "y")


# id -> (builder, rel_err tolerance of today's tests, would rel_err have passed it)
FAULTS = {
    "tnw_dB_drops_last_slab_at_k_slab_len_plus_1": (_fault_tnw_last_slab, 2e-2, True),
    "chain3f_y_drops_last_column_at_odd_d_out": (_fault_chain3f_last_column, 1e-5, False),
    "gemm_store_spills_into_ldc_gap": (_fault_gemm_spills_into_ldc_gap, 2e-2, True),
    "f16_y_truncated_instead_of_rne": (_fault_f16_y_truncated, 2e-2, True),
    "dA_drops_last_token_T8193": (lambda: _fault_drop_last_token(8193, "dA"), 2e-2, True),
    "dB_drops_last_token_T8193": (lambda: _fault_drop_last_token(8193, "dB"), 2e-2, True),
    "dbias_drops_last_token_T8193": (lambda: _fault_drop_last_token(8193, "dbias"), 2e-2, True),
    "dA_drops_last_token_T32769": (lambda: _fault_drop_last_token(32769, "dA"), 2e-2, True),
    "dB_drops_last_token_T32769": (lambda: _fault_drop_last_token(32769, "dB"), 2e-2, True),
    "dbias_drops_last_token_T32769": (lambda: _fault_drop_last_token(32769, "dbias"), 2e-2, True),
    "y_drops_last_column_of_ragged_d_in": (_fault_drop_last_column_of_y, 2e-2, False),
    "y_truncated_instead_of_rne": (lambda: _fault_y_store("trunc"), 2e-2, True),
    "y_rounded_twice_on_single_rounding_path": (lambda: _fault_y_store("twice"), 2e-2, True),
    "fp32_split_odd_lanes_take_even_lo_plane": (_fault_f32_odd_lo_plane, 1e-5, False),
    "ones_column_written_at_r_not_63": (_fault_ones_column_at_r, 2e-2, False),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_is_rejected(fault):
    build, tol, rel_err_blind = FAULTS[fault]
    out, ref, check = build()
    with pytest.raises(NumericsError) as e:
        check(out)
    passes_rel_err = rel_err(out, ref) < tol
    print(f"fault {fault}: rejected ({str(e.value)[:160]}); rel_err {rel_err(out, ref):.3g} "
          f"{'PASSES' if passes_rel_err else 'fails'} today's {tol:g}")
    # the documented gap: which faults the max-norm tolerance alone lets through
    assert passes_rel_err == rel_err_blind, (fault, rel_err(out, ref))


# ---- bounds added with the random sweep (tests/test_gpu_fuzz_elementwise.py) ------------------------------------------
def _emulate_f16_layer(T, d_in, d_out, r, s, seed, save_h=True):
    """An f16 layer as chain2_f16 / the f16 skinny-TN kernels compute it (fp32 sums of 64-wide blocks, one RNE_f16 per
    stored value), in the output layout of tests/test_gpu_elementwise._run_single."""
    g = torch.Generator().manual_seed(seed)
    x, A, B = _data((T, d_in), F16, g), _data((d_in, r), F16, g, 0.05), _data((r, d_out), F16, g, 0.05)
    bias, dy = _data((d_out,), F16, g, 0.1), _data((T, d_out), F16, g)
    h = rne(mm32(x, A) * s, F16)
    y = rne((mm32(h, B) + bias).float().double(), F16)
    dh = rne(mm32(dy, B.t()) * s, F16)
    dx = rne(mm32(dh, A.t()), F16)
    dA, dB = rne(mm32(x.t(), dh), F16), rne(mm32(h.t(), dy), F16)
    dbias = rne(mm32(torch.ones(1, T, dtype=torch.float64), dy).flatten(), F16)
    data = dict(x=x, A=A, B=B, bias=bias, dy=dy)
    out = dict(y=y, h=h_save_of(h, r) if save_h else None)
    if save_h:
        out.update(dx=dx, dA=dA, dB=dB, dbias=dbias)
    return data, out


@pytest.mark.parametrize("T,d_in,d_out,r,s,save_h", [(4097, 256, 264, 50, 0.5, True), (8193, 512, 136, 16, 2.0, True),
                                                      (65, 1000, 264, 63, 1.0, True), (4097, 256, 264, 50, 0.5, False)])
def test_f16_emulation_passes_elementwise_check_with_margin(T, d_in, d_out, r, s, save_h):
    """The f16 limits of test_gpu_elementwise._check (subnormal floor of hidden roundings, the inexact share of _rounded)
    pass an emulation of the f16 kernels with margin."""
    data, out = _emulate_f16_layer(T, d_in, d_out, r, s, seed=T + r, save_h=save_h)
    c = E.Case(f"emu_f16_T{T}_r{r}_{save_h}", F16, T, d_in, d_out, r, s=s, save_h=save_h)
    E._check(c, {k: v.to(F16) for k, v in data.items()}, out)
    st = {stage: v for (name, stage), v in E.WORST.items() if name == c.name}
    print(c.name, {k: (round(w, 3), None if i is None else round(100 * i, 4)) for k, (w, i) in st.items()})
    for stage, (w, inexact) in st.items():
        if inexact is None:
            assert w <= MARGIN, (stage, w)
        else:   # within one ulp everywhere, and off RNE(ref64) in at most 0.7 of the share _rounded allows
            assert w <= 1 and inexact <= MARGIN * E.ALLOWED[(c.name, stage)], (stage, w, inexact, E.ALLOWED[(c.name, stage)])


def mm3f_gemm(a, b, block=32):
    """gemm_x3.hip: a . b with both operands split into three truncated bf16 planes, six plane products, fp32 sums of
    32-wide K tiles."""
    pa, pb = split3(a), split3(b)
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k0 in range(0, a.shape[1], block):
        s = sum(pa[i][:, k0:k0 + block] @ pb[j][k0:k0 + block] for i in range(3) for j in range(3) if i + j <= 2)
        acc += s.float()
    return acc


@pytest.mark.parametrize("M,N,K,alpha,beta", [(256, 264, 2048, 1.0, 0.0), (128, 100, 300, -2.0, 0.5), (64, 72, 17, 0.5, 1.0)])
def test_gemm_x3_emulation_passes_with_margin(M, N, K, alpha, beta):
    """The fp32 sow_gemm bound (numerics.gemm_f32_bound) against an emulation of gemm_x3 with its fp32 epilogue."""
    g = torch.Generator().manual_seed(M + K)
    a, b = torch.randn(M, K, generator=g).double(), (torch.randn(K, N, generator=g) * 0.05).double()
    a, b = a.float().double(), b.float().double()
    c0 = torch.randn(M, N, generator=g).float().double()
    bias = (torch.randn(N, generator=g) * 0.1).float().double()
    acc = mm3f_gemm(a, b)
    out = (torch.tensor(alpha, dtype=torch.float32) * acc + torch.tensor(beta, dtype=torch.float32) * c0.float()
           + bias.float()).double()
    prod = a @ b
    ref = alpha * prod + beta * c0 + bias
    sq = alpha ** 2 * ((a * a) @ (b * b))
    w = check_bound(out, ref, gemm_f32_bound(ref, sq, alpha * prod, K, gemm_epilogue(prod, alpha, beta, c0, bias)), name="C")["worst"]
    print(f"gemm_x3 {M}x{N}x{K} alpha {alpha} beta {beta}: worst err/bound {w:.3f}")
    assert w <= MARGIN


def test_fp32_cancelled_dh_emulation_passes_with_margin():
    """The fp32 dA / dX bound of test_gpu_elementwise._check with the error of the fp32 dh sum: an emulation of the generic
    fp32 backward (dh = s dY B^T summed in fp32, dX = dh A^T, dA = x^T dh in fp32) at the sweep's r = 1, d_out = 80 layer,
    where dh cancels to ~1/1000 of its terms in many rows, passes with margin."""
    T, d_in, d_out, r, s = 4618, 304, 80, 1, 2.0
    g = torch.Generator().manual_seed(15)
    x = torch.randn(T, d_in, generator=g).float()
    A, B = (torch.randn(d_in, r, generator=g) * 0.05).float(), (torch.randn(r, d_out, generator=g) * 0.05).float()
    dy = torch.randn(T, d_out, generator=g).float()
    h = (x @ A) * s
    y = h @ B
    dh = (dy @ B.t()) * s
    out = dict(y=y.double(), h=h_save_of(h.double(), r), dx=(dh @ A.t()).double(), dA=(x.t() @ dh).double(),
               dB=(h.t() @ dy).double(), dbias=None)
    c = E.Case("emu_f32_r1_dout80", F32, T, d_in, d_out, r, bias=False, s=s)
    E._check(c, dict(x=x, A=A, B=B, bias=None, dy=dy), out)
    st = {stage: w for (name, stage), (w, _) in E.WORST.items() if name == c.name}
    print(c.name, {k: round(w, 3) for k, w in st.items()})
    assert max(st.values()) <= MARGIN, st


# ---- bit-exact checks on exact operands (tests/value_plan.py) ---------------------------------------------------------
def test_zero_tolerance_means_bit_exact_and_names_the_worst_element():
    g = torch.Generator().manual_seed(3)
    ref = torch.randint(-300, 300, (40, 70), generator=g).double() * 0.5
    out = rne(ref, BF16)
    st = check_rounded(out, ref, BF16, max_ulp=0, max_inexact=0, min_count=0, name="exact")
    assert st["worst"] == 0.0 and st["inexact"] == 0.0 and st["over"] == 0
    bad = out.clone()
    bad[3, 5] += float(ulp(bad[3:4, 5], BF16))
    with pytest.raises(NumericsError, match=r"worst element \(3, 5\) err/limit = inf.*1 of 2800 elements over the limit"):
        check_rounded(bad, ref, BF16, max_ulp=0, max_inexact=0, min_count=0, name="exact")
    check_rounded(bad, ref, BF16, name="default")           # one ulp in one element: within the default limits
    nan = out.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(NumericsError, match=r"worst element \(0, 0\)"):
        check_rounded(nan, ref, BF16, max_ulp=0, max_inexact=0, min_count=0, name="exact")


def test_one_token_in_32768_is_caught_only_on_exact_operands():
    """One token dropped from one column of dB (T = 32768), for eight columns in turn.  On Gaussian operands the fault
    moves an element by a fraction of an ulp unless the element happens to be small: some of the eight faulty dB pass the
    limits of check_rounded (rounding noise moves more elements than the fault does).  On the exact operands of
    value_plan.exact_layer the kernels' arithmetic (emulate_bf16) is exact, the zero-tolerance check passes, and every one
    of the eight faults fails it."""
    import value_plan as V
    T, d_in, d_out, r, s = 32768, 64, 64, 8, 0.5
    cols = range(0, 64, 8)

    def faulty_dB(h_live, dy, t0, col):
        dropped = dy.clone()
        dropped[t0, col] = 0
        return rne(mm32(h_live.t(), dropped), BF16)

    x, A, B, bias, dy, _ = _layer_inputs(T, d_in, d_out, r, 11)
    out = emulate_bf16(x, A, B, bias, dy, s)
    h = out["h_save"][:, :r]
    refs, bounds = layer_refs(x, A, B, bias, dy, s, h)
    passed = 0
    for col in cols:
        try:
            check_rounded(faulty_dB(h, dy, T // 2, col), refs["dB"], BF16, acc=bounds["dB"], name="dB")
            passed += 1
        except NumericsError:
            pass
    print(f"Gaussian operands: {passed} of {len(cols)} one-token faults pass the limits of check_rounded")
    assert passed >= 1

    c = FP.Layer("planted", "bf16", T, d_in, d_out, r, bias=True, s=s)
    d, f = V.exact_layer_proved(c)
    out = emulate_bf16(d["x"], d["A"], d["B"], d["bias"], d["dy"], s)
    zero = dict(max_ulp=0, max_inexact=0, min_count=0)
    for k in ("y", "dx", "dA", "dB", "dbias"):
        check_rounded(out[k], f[k], BF16, name=k, **zero)                 # the emulated kernels are exact on these operands
    assert torch.equal(out["h_save"][:, :r], f["h"]) and torch.equal(out["dh"], f["dh"])
    for col in cols:
        hit = torch.nonzero((d["dy"][T // 2:, col] != 0) & (f["h"][T // 2:] != 0).any(1))[0]
        with pytest.raises(NumericsError, match="dB"):
            check_rounded(faulty_dB(f["h"], d["dy"], T // 2 + int(hit), col), f["dB"], BF16, name="dB", **zero)
