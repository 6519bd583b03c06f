"""-m gpu: the kernels that write the model's weights and optimizer state, element by element against float64
(tests/step_numerics.py, tests/numerics.py): sow_adamw_flat, sow_ttadam_dense, sow_accumulate_batch, sow_qr_thin, and the
small helpers sow_cast_copy, sow_axpby, sow_zero_state, sow_tt_kron_core, sow_absmax, sow_small_inverse.

In the style of test_gpu_elementwise.py: every input is a view into a buffer whose neighbours hold NaN, every output has
sentinel guards on both sides, outputs and workspaces are poisoned (0xFF bytes) before the call, and three runs (poisoned,
zeroed, poisoned) must give bit-identical results.  In-place operands (the optimizer's p, m, v; an accumulator updated
with acc_beta = 1; A overwritten by its new orthonormal factor) are restored to their initial values before every run.
The -s output lists the worst err / limit of every checked output.
"""
import ctypes
import math
import time

import pytest
import torch

from numerics import check_bound, rne, to64, ulp
from step_numerics import U32, adamw_ref, check_qr, check_rank_update, check_rounded_noisy, check_step, ttadam_ref
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {F32: _lib.F32, BF16: _lib.BF16, F16: _lib.F16}
INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16, torch.uint8: torch.uint8}
GUARD = 64
SENTINEL = -7.25


def _bits(t):
    return t.view(INT[t.dtype])


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


class Arena:
    """Guarded inputs (NaN neighbours) and guarded outputs (sentinel guards, poisonable, optional initial values) of any
    dtype; `misalign` elements of offset break 16-byte alignment."""

    def __init__(self, misalign=0):
        self.misalign = misalign
        self.outs = []
        self.ins = []      # the input buffers stay alive as long as the arena: the C ABI holds only raw pointers

    def input(self, t, misalign=None):
        off = GUARD + (self.misalign if misalign is None else misalign)
        buf = torch.full((t.numel() + off + GUARD,), float("nan"), dtype=t.dtype, device=DEV)
        view = buf[off:off + t.numel()].view(t.shape)
        view.copy_(t.to(DEV))
        self.ins.append(buf)
        return view

    def output(self, shape, dtype, initial=None, misalign=None):
        off = GUARD + (self.misalign if misalign is None else misalign)
        n = math.prod(shape)
        buf = torch.full((n + off + GUARD,), SENTINEL, dtype=dtype, device=DEV)
        view = buf[off:off + n].view(shape)
        self.outs.append((buf, off, n, view, None if initial is None else initial.to(DEV, dtype)))
        return view

    def workspace(self, nbytes):
        ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=DEV)
        self.outs.append((ws, 0, ws.numel(), ws, None))
        return ws

    def fill(self, byte):
        for buf, off, n, view, init in self.outs:
            if init is not None:
                view.copy_(init)
            elif buf.dtype == torch.uint8:
                buf.fill_(byte)
            else:
                _bits(view).fill_(-1 if byte == 0xFF else 0)

    def check_guards(self, what):
        torch.cuda.synchronize()
        for buf, off, n, view, _ in self.outs:
            if buf.dtype == torch.uint8:
                continue
            for name, g in (("leading", buf[:off]), ("trailing", buf[off + n:])):
                assert not (g != SENTINEL).any(), f"{what}: a {name} output guard was overwritten"

    def run3(self, name, call, views):
        """call() three times on poisoned, zeroed, poisoned memory; the outputs `views` (dict) of the first run, on the
        CPU, after asserting bit-identity and intact guards."""
        runs = []
        for byte in (0xFF, 0x00, 0xFF):
            self.fill(byte)
            call()
            self.check_guards(f"{name} run {len(runs)}")
            runs.append({k: v.clone() for k, v in views.items()})
        for k, v in runs[0].items():
            for i in (1, 2):
                assert torch.equal(_bits(v), _bits(runs[i][k])), \
                    f"{name}: {k} of the {'zeroed' if i == 1 else 'repeated'} run differs from the poisoned run"
        return {k: v.cpu() for k, v in runs[0].items()}


WORST = {}


def _note(case, stats):
    for k, s in stats.items():
        WORST[(case, k)] = s["worst"]
    print(f"{case}: " + ", ".join(f"{k} {s['worst']:.3g}" + (f" ({100 * s['inexact']:.3f} % inexact)" if "inexact" in s
                                                            else "") for k, s in stats.items()))


# ---- sow_adamw_flat -----------------------------------------------------------------------------------------------------
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F16, F16), (F16, F32)]
N_OPT = 2048 * 256 + 12345          # past the 2048-block grid: the grid-stride loop wraps; not a multiple of 256


def _opt_data(n, pdtype, sdtype, step, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(n, generator=g, dtype=torch.float64) * 0.05).to(pdtype)
    gr = torch.randn(n, generator=g, dtype=torch.float64) * 1e-2
    t = n // 4
    gr[:t] = 0.0                                        # g = 0
    gr[t:2 * t] *= 1e-6                                 # tiny g: sqrt(v) near eps
    gr[3 * t:] *= 1e4 if pdtype != F16 else 1e3         # large g
    gr = gr.to(pdtype)
    if step == 1:
        m, v = torch.zeros(n, dtype=sdtype), torch.zeros(n, dtype=sdtype)
    else:                                               # resumed from given state
        m = (torch.randn(n, generator=g, dtype=torch.float64) * 1e-3).to(sdtype)
        v = (torch.rand(n, generator=g, dtype=torch.float64) * 1e-4).to(sdtype)
    return p, gr, m, v


@pytest.mark.parametrize("pdtype,sdtype", PAIRS, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("betas,step,wd,gs,misalign", [((0.9, 0.999), 1, 0.1, 0.5, 0), ((0.9, 0.95), 2, 0.0, 1.0, 1),
                                                       ((0.9, 0.999), 10, 0.0, 1.0, 0), ((0.9, 0.999), 1000, 0.1, 0.5, 1)])
def test_adamw_flat_against_fp64(pdtype, sdtype, betas, step, wd, gs, misalign):
    lib = _lib.load()
    hp = dict(lr=1e-3, betas=betas, eps=1e-8, wd=wd, step=step, grad_scale=gs)
    p0, g, m0, v0 = _opt_data(N_OPT, pdtype, sdtype, step, seed=step + 7 * misalign)
    ar = Arena(misalign)
    gd = ar.input(g)
    p, m, v = (ar.output((N_OPT,), t.dtype, initial=t) for t in (p0, m0, v0))
    out = ar.run3("adamw", lambda: _lib.check(lib.sow_adamw_flat(
        _p(p), _p(gd), _p(m), _p(v), N_OPT, hp["lr"], betas[0], betas[1], hp["eps"], wd, step, gs, DT[pdtype], DT[sdtype],
        _s()), "sow_adamw_flat"), dict(p=p, m=m, v=v))
    refs, mags = adamw_ref(p0, g, m0, v0, **hp)
    _note(f"adamw {pdtype}/{sdtype} betas={betas} step={step} wd={wd} gs={gs}",
          check_step(out, refs, mags, pdtype, sdtype, "adamw"))


# ---- sow_ttadam_dense ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp_v,wd", [(True, 0.0), (True, 0.01), (False, 0.01)])
def test_ttadam_dense_against_fp64(clamp_v, wd):
    lib = _lib.load()
    n = N_OPT
    p0, g, m0, v0 = _opt_data(n, F32, F32, 3, seed=31)
    if clamp_v:
        v0[::7] = -v0[::7]                              # negative moments of a lossy TT re-compression
    lr, betas, step = 1e-2, (0.9, 0.999), 3
    step_size = float(torch.tensor(lr * math.sqrt(1 - betas[1] ** step) / (1 - betas[0] ** step)).float())
    lr_wd = float(torch.tensor(lr * wd).float())
    ar = Arena()
    gd = ar.input(g)
    p, m, v = (ar.output((n,), F32, initial=t) for t in (p0, m0, v0))
    out = ar.run3("ttadam", lambda: _lib.check(lib.sow_ttadam_dense(
        _p(p), _p(gd), _p(m), _p(v), n, betas[0], betas[1], 1e-8, step_size, lr_wd, int(clamp_v), _s()),
        "sow_ttadam_dense"), dict(p=p, m=m, v=v))
    refs, mags = ttadam_ref(p0, g, m0, v0, betas=betas, eps=1e-8, step_size=step_size, lr_wd=lr_wd, clamp_v=clamp_v)
    _note(f"ttadam clamp_v={clamp_v} wd={wd}", check_step(out, refs, mags, F32, F32, "ttadam"))


# ---- sow_accumulate_batch -----------------------------------------------------------------------------------------------
def _acc_items(dtype):
    """120 items (> ACC_MAXB = 40 per rank-update launch, 116 QR items > QR_MAXB = 112 per panel launch)."""
    shapes = [(100, 259), (259, 100), (1001, 512), (512, 1001)]
    ranks = [1, 7, 50, 64]
    items = []
    for i in range(120):
        d_in, d_out = shapes[i % 4] if i < 8 else shapes[(i % 2)]   # the big shapes only in the first eight items
        r = ranks[i % 4]
        beta = 0.0 if i % 3 == 0 else 1.0
        draw = None if i % 30 == 29 else ("r", "more", "d_out")[i % 3]
        items.append(dict(d_in=d_in, d_out=d_out, r=r, beta=beta, scale=0.75 if i % 2 else -1.5, draw=draw,
                          alias=i % 2 == 0, zero=(1 + i % 17, 1 + i % 5)))
    return items


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=lambda d: str(d).split(".")[-1])
def test_accumulate_batch_against_fp64(dtype):
    lib = _lib.load()
    items = _acc_items(dtype)
    g = torch.Generator().manual_seed(5)
    ar = Arena()
    args = (_lib.AccumulateArgs * len(items))()
    keep, views = [], {}
    zpool = torch.full((len(items) * 64,), 0xAB, dtype=torch.uint8, device=DEV)
    for i, it in enumerate(items):
        d_in, d_out, r = it["d_in"], it["d_out"], it["r"]
        A0 = (torch.randn(d_in, r, generator=g) * 0.05).to(dtype)
        B0 = (torch.randn(r, d_out, generator=g) * 0.05).to(dtype)
        acc0 = (torch.randn(d_in, d_out, generator=g) * 0.01).to(dtype)
        acc = ar.output((d_in, d_out), dtype, initial=acc0 if it["beta"] else None)   # beta = 0: poisoned, never read
        Bd = ar.input(B0)
        r_new = r
        if it["draw"]:
            cols = {"r": r, "more": r + 5, "d_out": d_out}[it["draw"]]
            ld = cols + 3
            D0 = torch.randn(d_in, ld, generator=g).to(dtype)
            Dd = ar.input(D0)
            ws = ar.workspace(lib.sow_qr_workspace_bytes(d_in, cols, r_new, DT[dtype], 0) + 256)
        if it["draw"] and it["alias"]:
            A = ar.output((d_in, r), dtype, initial=A0)       # A_new = A: overwritten after the update read it
            A_new = A
        else:
            A = ar.input(A0)
            A_new = ar.output((d_in, r_new), dtype) if it["draw"] else None
        a = args[i]
        a.acc, a.A, a.B = _p(acc), _p(A), _p(Bd)
        a.d_in, a.d_out, a.r, a.r_new = d_in, d_out, r, r_new
        a.scale, a.acc_beta = it["scale"], it["beta"]
        if it["draw"]:
            a.draw, a.ld_draw, a.draw_cols, a.A_new = _p(Dd), ld, cols, _p(A_new)
            a.workspace, a.workspace_bytes = _p(ws), ws.numel()
        zoff, zlen = it["zero"]
        zoff = i * 64 + zoff                               # odd byte counts at misaligned starts
        a.zero, a.zero_bytes = zpool.data_ptr() + zoff, zlen
        views[f"acc{i}"] = acc
        if it["draw"]:
            views[f"Anew{i}"] = A_new
        keep.append((it, A0, B0, acc0, D0[:, :cols] if it["draw"] else None, (zoff, zlen)))

    def call():
        zpool.fill_(0xAB)
        _lib.check(lib.sow_accumulate_batch(args, len(items), DT[dtype], _s()), "sow_accumulate_batch")
    out = ar.run3(f"accumulate {dtype}", call, views)
    zp = zpool.cpu()
    mask = torch.zeros_like(zp, dtype=torch.bool)
    worst = {}
    for i, (it, A0, B0, acc0, draw, (zoff, zlen)) in enumerate(keep):
        mask[zoff:zoff + zlen] = True
        st = check_rank_update(out[f"acc{i}"], acc0, A0, B0, it["scale"], it["beta"], dtype, name=f"item {i} acc")
        worst["acc"] = max(worst.get("acc", 0.0), st["worst"])
        if draw is not None:
            # Q[:, :r_new] of the draw: orthonormal, and column by column LAPACK's Q of draw[:, :r_new]
            sq = check_qr(draw[:, :it["r"]], out[f"Anew{i}"], None, it["r"], dtype, name=f"item {i} A_new")
            for k, s in sq.items():
                worst[k] = max(worst.get(k, 0.0), s["worst"])
    assert (zp[mask] == 0).all(), "zero: a byte of a zeroed span is not 0"
    assert (zp[~mask] == 0xAB).all(), "zero: a byte outside the zeroed spans was written"
    print(f"accumulate {dtype}: worst err/limit {worst}")


# ---- sow_qr_thin --------------------------------------------------------------------------------------------------------
QR_CASES = [  # (m, n, k, in, out, need_r, extra ld, scale)
    (512, 512, 512, F32, F32, 1, 0, 1.0), (1376, 512, 512, BF16, F32, 1, 5, 1.0), (512, 1376, 512, F32, BF16, 1, 0, 1.0),
    (512, 1376, 512, F16, F16, 1, 3, 1.0), (1376, 512, 512, F32, F16, 0, 0, 1.0), (1001, 1001, 1001, F32, F32, 1, 7, 1.0),
    (1001, 300, 600, F32, F32, 1, 0, 1.0), (1001, 300, 600, BF16, BF16, 1, 0, 1.0), (1001, 600, 300, F16, F32, 1, 1, 1.0),
    (300, 700, 100, BF16, F16, 1, 0, 1.0), (259, 100, 50, F32, BF16, 0, 2, 1.0),
    (512, 256, 256, F32, F32, 1, 0, 1e-12), (512, 256, 256, BF16, F32, 1, 0, 1e12),
]


def _run_qr(W0, k, out_dtype, need_r, extra_ld, name):
    lib = _lib.load()
    m, n = W0.shape
    ldw = n + extra_ld
    ar = Arena()
    Wb = ar.input(torch.cat([W0, torch.zeros(m, extra_ld, dtype=W0.dtype)], 1) if extra_ld else W0)
    Q = ar.output((m, k), out_dtype)
    R = ar.output((k, n), out_dtype) if need_r else None
    ws = ar.workspace(lib.sow_qr_workspace_bytes(m, n, k, DT[W0.dtype], need_r))
    views = dict(Q=Q) if R is None else dict(Q=Q, R=R)
    t0 = time.time()
    out = ar.run3(name, lambda: _lib.check(lib.sow_qr_thin(_p(Wb), ldw, m, n, DT[W0.dtype], k, _p(Q), k, _p(R), n,
                                                           DT[out_dtype], _p(ws), ws.numel(), _s()), "sow_qr_thin"), views)
    return out, (time.time() - t0) / 3


@pytest.mark.parametrize("m,n,k,din,dout,need_r,extra_ld,scale", QR_CASES)
def test_qr_thin_against_fp64(m, n, k, din, dout, need_r, extra_ld, scale):
    """Q_out [m, k], R_out [k, n].  For n < k <= m the panel factors kc = n columns: Q_out[:, :n] is qr_weight's Q (which
    returns only min(m, n) columns), Q_out[:, n:k] continues it with LAPACK's complete-mode columns H_0 .. H_{n-1} e_j, and
    the rows n..k-1 of R_out are 0."""
    W0 = (torch.randn(m, n, generator=torch.Generator().manual_seed(m + n + k)) * scale).to(din)
    out, dt = _run_qr(W0, k, dout, need_r, extra_ld, f"qr {m}x{n} k={k}")
    st = check_qr(W0, out["Q"], out.get("R"), k, dout, name=f"qr {m}x{n} k={k}")
    _note(f"qr {m}x{n} k={k} {din}->{dout} need_r={need_r} scale={scale:g} ({1e3 * dt:.0f} ms/call)", st)


def test_qr_thin_large_k():
    """k = 2048 of a 2048 x 5461 matrix (the widest prepare_sow(decompose='qr') factor of llama-7b-like shapes)."""
    W0 = torch.randn(2048, 5461, generator=torch.Generator().manual_seed(1)).to(BF16)
    out, dt = _run_qr(W0, 2048, F32, 1, 0, "qr 2048x5461")
    print(f"qr 2048 x 5461, k = 2048: {dt:.2f} s per call")
    st = check_qr(W0, out["Q"], out["R"], 2048, F32, name="qr 2048x5461", against_lapack=False)
    _note(f"qr 2048x5461 k=2048 ({dt:.2f} s/call)", st)


@pytest.mark.parametrize("kind", ["zero_column", "repeated_column"])
def test_qr_thin_rank_deficient(kind):
    """Only the well-defined parts (R's zero lower triangle, backward error, orthogonality, the R tail) and no NaN."""
    W0 = torch.randn(300, 120, generator=torch.Generator().manual_seed(9))
    if kind == "zero_column":
        W0[:, 17] = 0
    else:
        W0[:, 40] = W0[:, 12]
    out, _ = _run_qr(W0, 80, F32, 1, 0, f"qr {kind}")
    _note(f"qr {kind}", check_qr(W0, out["Q"], out["R"], 80, F32, name=f"qr {kind}", against_lapack=False))


# ---- small kernels ------------------------------------------------------------------------------------------------------
def _cast_sources():
    """16-bit sources: every bit pattern.  fp32 source: the rounding midpoints of a sample of bf16 and f16 values, the
    fp32 neighbours on both sides, the f16 overflow edge, f16 subnormals down to 2^-25, fp32 subnormals."""
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    g = torch.Generator().manual_seed(3)
    vals = []
    for dt, lo in ((BF16, -120), (F16, -24)):
        x = torch.ldexp(torch.rand(4000, generator=g, dtype=torch.float64) + 1, torch.randint(lo, 15, (4000,), generator=g))
        x = torch.cat([x, -x]).to(dt).double()
        mid = x + ulp(x, dt) / 2                                 # ties between x and its successor: to even and to odd
        for v in (mid.float(), torch.nextafter(mid.float(), torch.tensor(math.inf)),
                  torch.nextafter(mid.float(), torch.tensor(-math.inf))):
            vals.append(v)
    edge = torch.tensor([65519.996, 65520.0, -65520.0, 65504.0, 65536.0, 1e30, -1e-30, 2.0 ** -25, 2.0 ** -24,
                         3 * 2.0 ** -26, 2.0 ** -14 * 0.999, 0.0, -0.0, math.inf, -math.inf, float("nan")])
    sub = torch.ldexp(torch.rand(999, generator=g, dtype=torch.float64) + 1, torch.randint(-149, -126, (999,),
                                                                                             generator=g)).float()
    f32 = torch.cat(vals + [edge, sub, -sub])
    return {BF16: pat.view(BF16), F16: pat.view(F16), F32: f32}


def _same(a, b):
    both_nan = torch.isnan(a.float()) & torch.isnan(b.float())
    return bool(((_bits(a) == _bits(b)) | both_nan).all())


@pytest.mark.parametrize("src", [F32, BF16, F16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("dst", [F32, BF16, F16], ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("layout", ["flat", "misaligned", "strided"])
def test_cast_copy_bit_exact(src, dst, layout):
    lib = _lib.load()
    x = _cast_sources()[src]
    n = x.numel() - x.numel() % 8 + 5                          # flat branch: n % 8 != 0
    x = torch.cat([x, x[:5]])[:n]
    ref = x.to(dst)
    if layout == "strided":
        cols = 129
        rows = n // cols
        x, ref = x[:rows * cols].view(rows, cols), ref[:rows * cols].view(rows, cols)
        ar = Arena()
        xs = ar.input(torch.cat([x, torch.zeros(rows, 3, dtype=src)], 1))
        y = ar.output((rows, cols + 2), dst)
        out = ar.run3("cast", lambda: _lib.check(lib.sow_cast_copy(_p(xs), cols + 3, DT[src], _p(y), cols + 2, DT[dst], rows,
                                                                   cols, _s()), "sow_cast_copy"), dict(y=y[:, :cols]))["y"]
        # the last run was on poisoned memory: the two padding elements of every row must still hold the poison
        assert (_bits(y[:, cols:]) == -1).all(), "cast: the row padding of a strided output was written"
    else:
        ar = Arena(1 if layout == "misaligned" else 0)
        xs = ar.input(x)
        y = ar.output((n,), dst)
        out = ar.run3("cast", lambda: _lib.check(lib.sow_cast_copy(_p(xs), n, DT[src], _p(y), n, DT[dst], 1, n, _s()),
                                                 "sow_cast_copy"), dict(y=y))["y"]
    bad = ~(((_bits(out) == _bits(ref)) | (torch.isnan(out.float()) & torch.isnan(ref.float()))))
    assert not bad.any(), (f"{src}->{dst} {layout}: {int(bad.sum())} elements differ from torch's cast, first "
                           f"{x.reshape(-1)[bad.reshape(-1)][:4].tolist()} -> {out.reshape(-1)[bad.reshape(-1)][:4].tolist()} "
                           f"(torch {ref.reshape(-1)[bad.reshape(-1)][:4].tolist()})")


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: str(d).split(".")[-1])
def test_axpby_single_rounding(dtype):
    lib = _lib.load()
    n = 2048 * 256 + 77
    g = torch.Generator().manual_seed(4)
    x0, y0 = torch.randn(n, generator=g).to(dtype), torch.randn(n, generator=g).to(dtype)
    a, b = 0.7, -1.3
    ar = Arena()
    x = ar.input(x0)
    y = ar.output((n,), dtype, initial=y0)
    out = ar.run3("axpby", lambda: _lib.check(lib.sow_axpby(_p(x), _p(y), n, a, b, DT[dtype], _s()), "sow_axpby"),
                  dict(y=y))["y"]
    af, bf = float(torch.tensor(a).float()), float(torch.tensor(b).float())   # the fp32 scalars of the C ABI
    ref = af * to64(x0) + bf * to64(y0)
    # fp32: a*x and b*y rounded (u each of their magnitudes), the sum rounded (one ulp)
    noise = 2 * U32 * (abs(af) * to64(x0).abs() + abs(bf) * to64(y0).abs())
    st = check_bound(out, ref, ulp(ref, F32) + noise, name="axpby") if dtype == F32 else \
        check_rounded_noisy(out, ref, dtype, noise + ulp(ref, F32), name="axpby")
    _note(f"axpby {dtype}", dict(y=st))
    # b = 0 on a NaN y: y is not read, the result is a * x
    ar = Arena()
    x = ar.input(x0)
    y = ar.output((n,), dtype)
    out = ar.run3("axpby b=0", lambda: _lib.check(lib.sow_axpby(_p(x), _p(y), n, a, 0.0, DT[dtype], _s()), "sow_axpby"),
                  dict(y=y))["y"]
    ref = af * to64(x0)
    assert not torch.isnan(out.float()).any(), "axpby b = 0: the NaN of y leaked"
    if dtype == F32:
        assert torch.equal(to64(out), rne(ref, F32)), "axpby b = 0: not RNE(a x)"   # one product, one rounding
    else:   # a x rounded to fp32, then to the 16-bit dtype
        _note(f"axpby b=0 {dtype}", dict(y=check_rounded_noisy(out, ref, dtype, ulp(ref, F32), name="axpby b=0")))


def test_zero_state_spans():
    """Byte counts 1..17 at misaligned starts, a few long spans, 60 buffers (> MT_MAX = 48 per launch)."""
    lib = _lib.load()
    pool = torch.full((1 << 20,), 0xAB, dtype=torch.uint8, device=DEV)
    spans, pos = [], 0
    for i in range(60):
        n = 1 + i % 17 if i < 51 else [1001, 4096, 70001, 3, 16, 17, 31, 65, 100003][i - 51]
        start = pos + 1 + (i % 15)
        spans.append((start, n))
        pos = start + n + 16
    ptrs = (ctypes.c_void_p * len(spans))(*[pool.data_ptr() + s for s, _ in spans])
    sizes = (ctypes.c_int64 * len(spans))(*[n for _, n in spans])
    _lib.check(lib.sow_zero_state(ptrs, sizes, len(spans), _s()), "sow_zero_state")
    out = pool.cpu()
    mask = torch.zeros_like(out, dtype=torch.bool)
    for s, n in spans:
        mask[s:s + n] = True
    assert (out[mask] == 0).all(), "a byte of a zeroed span is not 0"
    assert (out[~mask] == 0xAB).all(), "a byte outside the spans was written"


def test_tt_kron_core_bit_exact():
    """An fp32 product is correctly rounded on both sides: bit-exact against the CPU."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(6)
    ra0, rb0, ij, ra1, rb1 = 3, 5, 4 * 7, 6, 9
    A0, B0 = torch.randn(ra0, ij, ra1, generator=g), torch.randn(rb0, ij, rb1, generator=g)
    ar = Arena()
    A, B = ar.input(A0), ar.input(B0)
    out = ar.output((ra0 * rb0, ij, ra1 * rb1), F32)
    res = ar.run3("kron", lambda: _lib.check(lib.sow_tt_kron_core(_p(A), _p(B), _p(out), ra0, rb0, ij, ra1, rb1, _s()),
                                             "sow_tt_kron_core"), dict(o=out))["o"]
    ref = torch.einsum("aeb,ced->acebd", A0.double(), B0.double()).reshape(ra0 * rb0, ij, ra1 * rb1).float()
    assert torch.equal(_bits(res), _bits(ref))


def test_absmax_bit_exact_and_nan():
    """max |x| exactly.  A NaN element is dropped (fmaxf returns the other operand): the result is the max over the
    non-NaN elements, where torch.amax would return NaN -- pinned here and in include/sow_amd.h."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(8)
    for n in (1, 63, 1024, 1025, 100003):
        x0 = torch.randn(n, generator=g) * 3
        ar = Arena()
        x = ar.input(x0)
        o = ar.output((1,), F32)
        res = ar.run3("absmax", lambda: _lib.check(lib.sow_absmax(_p(x), n, _p(o), _s()), "sow_absmax"), dict(o=o))["o"]
        assert float(res) == float(x0.abs().max()), n
        x0[n // 2] = float("nan")
        x.copy_(x0.to(DEV))
        res = ar.run3("absmax nan", lambda: _lib.check(lib.sow_absmax(_p(x), n, _p(o), _s()), "sow_absmax"), dict(o=o))["o"]
        others = torch.cat([x0[:n // 2], x0[n // 2 + 1:]])
        assert float(res) == (float(others.abs().max()) if n > 1 else 0.0), n


def test_small_inverse_residual():
    """r = 1..16, batch 1000 (not a multiple of 64): |A X - I| <= 8 r u P|L||U| |X| per element (Gauss-Jordan with partial
    pivoting, Higham, Accuracy and Stability, Thm 14.5, with the LU factors of the same pivoting); r = 17 refused."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(10)
    worst = 0.0
    for r in range(1, 17):
        A0 = torch.randn(1000, r, r, generator=g)
        ar = Arena()
        A = ar.input(A0)
        X = ar.output((1000, r, r), F32)
        res = ar.run3("inverse", lambda: _lib.check(lib.sow_small_inverse(_p(A), _p(X), 1000, r, _s()),
                                                    "sow_small_inverse"), dict(X=X))["X"]
        A64, X64 = A0.double(), res.double()
        P, L, U = torch.linalg.lu(A64)
        E = A64 @ X64 - torch.eye(r, dtype=torch.float64)
        lim = 8 * r * U32 * (P @ (L.abs() @ U.abs())) @ X64.abs()
        st = check_bound(E, torch.zeros_like(E), lim, name=f"A X - I r={r}")
        worst = max(worst, st["worst"])
    print(f"small_inverse: worst err/limit {worst:.3g}")
    buf = torch.zeros(17 * 17, device=DEV)
    assert lib.sow_small_inverse(_p(buf), _p(buf), 1, 17, _s()) == _lib.ERR_UNSUPPORTED
