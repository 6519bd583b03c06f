"""Operands of the skinny-forward cases of tests/fuzz_plan.py (a plain module: torch on the CPU, no GPU) -- shared by
tests/test_gpu_fuzz_elementwise.py and tests/test_fuzz_plan_cpu.py.

* off_ties: the tie-clearing step of tests/test_gpu_fp4_acc.py for a layer with any accumulator or none.  The float64
  reference (test_gpu_skinny._reference) rounds the EXACT h = s x A; the kernel rounds an fp32 sum, and where the exact value
  lies within that sum's noise of a rounding midpoint the two may round apart -- y then moves by ulp(h) B[j, n], which is no
  error of the kernel and which the comparator has no term for.  The step moves such projections off their ties, by one ulp
  of single elements of A, decided from the operands alone before anything runs.
* operands: the Gaussian operands of a fuzz_plan.Skinny case (test_gpu_skinny._gauss), W replaced by its quantisation where
  the kind says so, clear of ties, with the condition test_gpu_fp4_acc sets: at most 1 % of A's elements moved.
* fp32_master: fp32 values that round to given numbers of the compute dtype, most of them no numbers of it.
"""
import torch

from numerics import bound, fp32_floor, rne, to64, ulp

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def off_ties(dtype, d):
    """The operands `d` (x, A, B, bias or None, W or None (a quantised W: W^), s; other keys pass through) with the projections
    that matter moved off rounding ties.  An element (t, j) of h MATTERS when a flip of its rounding would move some y of its row
    by more than an eighth of the comparator's own bound; while one that matters is within the noise of a tie (fewer than 64 fp32
    roundings: test_gpu_fp8_acc._tie_margin), one more element of column j of A is moved by one ulp (each element at most once),
    which shifts the column's h by about s x[t, k] ulp(A).  The terms of y that A does not enter -- x W, its squares, the bias --
    are formed once.  Returns (d, elements moved)."""
    A = d["A"].clone()
    d = dict(d, A=A)
    x, B, sc = to64(d["x"]), to64(d["B"]), d["s"]
    xx, BB = x * x, B * B
    base, base_sq = 0.0, 0.0
    if d.get("W") is not None:
        W = to64(d["W"])
        base, base_sq = x @ W, xx @ (W * W)
        del W
    n_y = x.shape[1] + max(A.shape[1], 64)
    nxt = [0] * A.shape[1]
    for _ in range(4 * A.shape[0]):
        A64 = to64(A)
        h_exact = sc * (x @ A64)
        h = rne(h_exact, dtype)
        y_ref = h @ B + base
        if d.get("bias") is not None:
            y_ref = y_ref + to64(d["bias"])
        bnd = bound(y_ref, dtype, fp32_floor((h * h) @ BB + base_sq, n_y))
        half, noise = ulp(h_exact, dtype) / 2, fp32_floor(sc * sc * xx @ (A64 * A64), 64)
        near = (half - (h_exact - h).abs()) <= noise
        impact = torch.stack([2 * half[t] * (B.abs() / bnd[t]).amax(dim=1) for t in range(h.shape[0])])
        cols = sorted(set(torch.nonzero(near & (half > noise) & (impact > 0.125))[:, 1].tolist()))
        if not cols:
            return d, sum(nxt)
        for j in cols:
            assert nxt[j] < A.shape[0], f"column {j} of h stays on a rounding tie"
            A[nxt[j]:nxt[j] + 1, j].view(torch.int16).add_(1)
            nxt[j] += 1
    raise AssertionError("the projections stay on rounding ties")


def operands(c, quantise=None, x=None):
    """CPU operands of the fuzz_plan.Skinny case c, clear of ties: x, A, B, bias, W (None without an accumulator; W^ for the
    code formats, with "q" / "e": what the kernel reads, from quantise(W) -> (codes, scales, W^)), s.  x: the input of a call
    whose layers share one (given before the ties are cleared: they depend on it).  Returns (operands, elements of A moved)."""
    import test_gpu_skinny as S
    dtype = DT[c.dtype]
    d = dict(S._gauss(dtype, c.T, c.d_in, c.d_out, c.r, c.bias, "dense" if c.kind != "none" else "none", seed=c.seed), s=c.s)
    if x is not None:
        d["x"] = x
    if c.kind in ("e4m3", "mxfp4"):
        codes, scales, what = quantise(d["W"])
        d.update(W=what, q=codes, e=scales)
    d, moved = off_ties(dtype, d)
    assert moved <= d["A"].numel() // 100, f"{c.name}: {moved} of {d['A'].numel()} elements of A moved off ties"
    return d, moved


def fp32_master(t):
    """fp32 values that round (to nearest even) to the numbers `t` of a 16-bit dtype: element i holds, by i mod 4, t itself, a
    quarter of the way to its neighbour n away from zero (rounds down to t), an eighth of that gap towards zero (rounds up to t;
    an eighth, because the gap below a power of two is half the gap above), or -- where the last bit of t is even -- the exact
    midpoint (t + n) / 2, a tie that goes to t.  Zeros and the largest finite numbers stay as they are."""
    bits = t.view(torch.int16)
    n = (bits + 1).view(t.dtype)
    tf, nf = t.float().flatten(), n.float().flatten()
    ok = (tf != 0) & torch.isfinite(nf)
    gap = torch.where(ok, nf - tf, torch.zeros_like(tf))
    sel = torch.arange(tf.numel()) % 4
    even = (bits.flatten() & 1) == 0
    out = torch.where(sel == 1, tf + gap / 4, torch.where(sel == 2, tf - gap / 8, torch.where((sel == 3) & even, tf + gap / 2, tf)))
    out = out.view(t.shape)
    assert torch.equal(out.to(t.dtype).view(torch.int16), bits), "a master does not round to its number"
    return out
