"""The seeded sweep of tests/test_gpu_rows_sweep.py (a plain module: importable without a GPU, no torch): the 33 - 64-row forward
(sow_forward_skinny_rows) and the short-batch pairs (sow_forward_short / sow_backward_short and their forms on E4M3 / MXFP4
codes) over the classes of their slab plans.  A seed and a draw object of its own: fuzz_plan.plan() and its streams are not touched.

* mirrors of the three C planning functions of skinny_fwd.hip (skinny_rows_plan, short_rows_plan, short_codes_plan) and of the
  five workspace queries of api.hip built on them; the plan_ws(...).total term of two of them is taken from sow_workspace_bytes
  (`base`), not derived again;
* class functions a test can count over any list of cases: slab length, tail class of either direction, column class of the last
  range, "more than 16 slabs", row-block count, rows of the last block, rank tiles;
* plan(seed): four case lists -- rows, short, short_codes, short_groups -- whose names carry the slab plan (KS{ks}x{S}).

A short case is drawn LED by one direction: the led direction's slab length, tail class, column class and slab count are what its
spec names; the other direction takes what falls out.  Coverage is counted from the drawn cases (tests/test_rows_plan_cpu.py).
"""
from __future__ import annotations

import dataclasses
import random
from typing import List

from fuzz_plan import SK_R_EDGES, al256, cdiv, sk_cn, sk_step, skinny_plan

SEED = 20261023
KQ_FWD, KQ_BWD = 128, 256            # SK_SHORT_KQ_FWD / SK_SHORT_KQ_BWD: a round of the four waves, forward / transposed form
KS_MAX48, KS_MAX64 = 768, 512        # SK_KS_MAX48 / SK_KS_MAX64
ROWS_WANT, ROWS_WANT8 = 512, 256     # SOW_SKINNY_ROWS_WANT / _WANT8
SHORT_WANT, SHORT_WANT8 = 512, 256   # SOW_SKINNY_SHORT_WANT / _WANT8
SK_MAXL = SK_BS = 16                 # entries of a launch pair; slab partials phase B requests up front
SHORT_MAX = 1024                     # SOW_SHORT_ROWS_MAX
KINDS = ("dense", "e4m3", "mxfp4", "none")
CODES = ("e4m3", "mxfp4")
ROWS_T_EDGES = (33, 47, 48, 49, 63, 64)
SHORT_T_FIXED = (1, 16, 17, 32, 33, 47, 48, 49, 63, 64, 65, 112, 113, 961, 1023, 1024)
LAST_ROWS = (1, 16, 17, 32, 33, 47, 48, 49, 63, 64)
FWD_TAILS = ("kgroup", "partial", "full", ">512")     # ">512": sow_forward_skinny_rows at T <= 48 only
BWD_TAILS = ("kgroup", "half", "pair+", "idle", "full")
COLS = ("lt", "8", "cn-8", "0", "other")
COLS_FP4_BWD = ("0", "32", "=32")
BLOCKS = ("1", "2", "3-15", "16")
SCALES = (1.0, 0.5, 0.25)


# ---- mirrors of the C planning functions (skinny_fwd.hip): (slab count S, slab length KS, column ranges) ------------------------
def skinny_rows_plan(T, d_in, d_out, kind):
    if T <= 32:
        return skinny_plan(d_in, d_out, kind)
    nc = cdiv(d_out, sk_cn(kind)) if kind != "none" else 0
    want = cdiv(ROWS_WANT8 if kind in CODES else ROWS_WANT, nc) if nc else 32
    ks = min(max(cdiv(cdiv(d_in, want), 128) * 128, 128), KS_MAX64 if T > 48 else KS_MAX48)
    return cdiv(d_in, ks), ks, nc


def short_rows_plan(T, K, N, kq):
    """kq = KQ_FWD for the forward (K = d_in, N = d_out), KQ_BWD for the data gradient (K = d_out, N = d_in)."""
    nblk, nc = cdiv(T, 64), cdiv(N, 64)
    want = cdiv(SHORT_WANT, nc * max(nblk, 1))
    ks = min(max(cdiv(cdiv(K, want), kq) * kq, kq), KS_MAX64)
    return cdiv(K, ks), ks, nc


def short_codes_plan(T, K, N):
    nblk, nc = cdiv(T, 64), cdiv(N, 128)
    want = cdiv(SHORT_WANT8, nc * max(nblk, 1))
    ks = min(max(cdiv(cdiv(K, want), KQ_FWD) * KQ_FWD, KQ_FWD), KS_MAX64)
    return cdiv(K, ks), ks, nc


def fwd_plan(kind, T, d_in, d_out):
    """The forward's plan of a short case by the format of its accumulator."""
    return short_codes_plan(T, d_in, d_out) if kind in CODES else short_rows_plan(T, d_in, d_out, KQ_FWD)


def bwd_plan(T, d_in, d_out):
    """The data gradient's plan (the plain geometry for every format): the contraction runs over d_out."""
    return short_rows_plan(T, d_out, d_in, KQ_BWD)


# ---- mirrors of the workspace queries (api.hip); 0 outside the admitted set of shapes ----------------------------------------------
def _widths_ok(d_in, d_out, r, kind):
    return d_in > 0 and d_out > 0 and 1 <= r <= 64 and d_in % 8 == 0 and d_out % 8 == 0 and (kind != "mxfp4" or d_in % 32 == 0)


def _part(T, N, S):
    """The slab partials of one direction: Py [S][T][N] and Ph [S][T][64] in fp32, each 256-aligned."""
    return al256(S * T * N * 4) + al256(S * T * 64 * 4)


def _plan_total(base):
    """plan_ws(...).total from sow_workspace_bytes of an unflagged dtype, which adds 256 bytes of alignment slack to it."""
    return base - 256


def rows_ws_bytes(T, d_in, d_out, r, kind):
    """sow_forward_skinny_rows_workspace_bytes."""
    if not (1 <= T <= 64 and kind in KINDS and _widths_ok(d_in, d_out, r, kind)):
        return 0
    S = skinny_rows_plan(T, d_in, d_out, kind)[0]
    return 256 + (al256(S * T * d_out * 4) if kind != "none" else 0) + al256(S * T * 64 * 4)


def forward_short_ws_bytes(T, d_in, d_out, r, kind="dense"):
    """sow_forward_short_workspace_bytes."""
    if not (1 <= T <= SHORT_MAX and kind == "dense" and _widths_ok(d_in, d_out, r, kind)):
        return 0
    return 256 + _part(T, d_out, short_rows_plan(T, d_in, d_out, KQ_FWD)[0])


def short_ws_bytes(T, d_in, d_out, r, base, kind="dense"):
    """sow_short_workspace_bytes; base = sow_workspace_bytes(T, d_in, d_out, r, 0, SOW_ACC_DENSE, dtype)."""
    if not (1 <= T <= SHORT_MAX and kind == "dense" and _widths_ok(d_in, d_out, r, kind)):
        return 0
    return _plan_total(base) + max(_part(T, d_out, short_rows_plan(T, d_in, d_out, KQ_FWD)[0]), _part(T, d_in, bwd_plan(T, d_in, d_out)[0])) + 256


def forward_short_codes_ws_bytes(T, d_in, d_out, r, kind):
    """sow_forward_short_codes_workspace_bytes."""
    if not (1 <= T <= SHORT_MAX and kind in CODES and _widths_ok(d_in, d_out, r, kind)):
        return 0
    return 256 + _part(T, d_out, short_codes_plan(T, d_in, d_out)[0])


def short_codes_ws_bytes(T, d_in, d_out, r, kind, base):
    """sow_short_codes_workspace_bytes; base as for short_ws_bytes (the weight phases are called with SOW_ACC_DENSE)."""
    if not (1 <= T <= SHORT_MAX and kind in CODES and _widths_ok(d_in, d_out, r, kind)):
        return 0
    return _plan_total(base) + max(_part(T, d_out, short_codes_plan(T, d_in, d_out)[0]), _part(T, d_in, bwd_plan(T, d_in, d_out)[0])) + 256


# ---- classes ---------------------------------------------------------------------------------------------------------------------------
def fwd_tail_classes(K, S, ks, step):
    """FWD_TAILS of the last slab of a forward: one k-group (8, or 32 for MXFP4); otherwise no multiple of 128 (a partial round of
    the four waves); above 512 (a fifth k-step: slabs of 640 and 768 only); a whole slab."""
    tail = K - (S - 1) * ks
    out = set()
    if tail == step:
        out.add("kgroup")
    elif tail % 128:
        out.add("partial")
    if tail > 512:
        out.add(">512")
    if tail == ks:
        out.add("full")
    return out


def bwd_tail_class(d_out, S, ks):
    """BWD_TAILS of the last slab of a data gradient (the transposed form takes k in pairs of k-steps per wave, 64 deep, and rounds
    of 256): one k-group; one k-step of a pair filled and the other not or partly; a whole pair and more; whole pairs with idle
    waves; a whole slab.  None: whole rounds short of the slab."""
    tail = d_out - (S - 1) * ks
    if tail == 8:
        return "kgroup"
    if tail == ks:
        return "full"
    if 8 <= tail % 64 <= 32:
        return "half"
    if 40 <= tail % 64 <= 56:
        return "pair+"
    if tail % 64 == 0 and tail % 256:
        return "idle"
    return None


def col_class(N, cn):
    """COLS of the last column range of N columns in ranges of cn."""
    if N < cn:
        return "lt"
    return {8: "8", cn - 8: "cn-8", 0: "0"}.get(N % cn, "other")


def bwd_col_class(d_in, kind):
    """The data gradient writes d_in columns in ranges of 64; on MXFP4 a group of 32 is whole or absent: COLS_FP4_BWD."""
    if kind != "mxfp4":
        return col_class(d_in, 64)
    return "=32" if d_in == 32 else str(d_in % 64)


def block_class(T):
    n = cdiv(T, 64)
    return "1" if n == 1 else "2" if n == 2 else "16" if n == 16 else "3-15"


def last_rows(T):
    return T - (cdiv(T, 64) - 1) * 64


def rank_tiles(r):
    return cdiv(r, 16)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Rows:
    name: str
    dtype: str                  # "bf16" | "f16"
    kind: str                   # KINDS
    T: int
    d_in: int
    d_out: int
    r: int
    bias: bool
    s: float
    f32: bool                   # fp32 factors (SOW_PARAM_F32 | SOW_ACC_NATIVE)
    seed: int

    def plan(self):
        return skinny_rows_plan(self.T, self.d_in, self.d_out, self.kind)

    def tails(self):
        S, ks, _ = self.plan()
        return fwd_tail_classes(self.d_in, S, ks, sk_step(self.kind))

    def col(self):
        return col_class(self.d_out, sk_cn(self.kind))


@dataclasses.dataclass
class Short:
    name: str
    dtype: str
    kind: str                   # "dense" | "e4m3" | "mxfp4"
    T: int
    d_in: int
    d_out: int
    r: int
    bias: bool
    s: float
    seed: int
    led: str = ""               # "f" | "b": the direction the case was drawn for

    def fwd(self):
        return fwd_plan(self.kind, self.T, self.d_in, self.d_out)

    def bwd(self):
        return bwd_plan(self.T, self.d_in, self.d_out)

    def fwd_tails(self):
        S, ks, _ = self.fwd()
        return fwd_tail_classes(self.d_in, S, ks, sk_step(self.kind))

    def bwd_tail(self):
        S, ks, _ = self.bwd()
        return bwd_tail_class(self.d_out, S, ks)

    def fwd_col(self):
        return col_class(self.d_out, sk_cn(self.kind))

    def bwd_col(self):
        return bwd_col_class(self.d_in, self.kind)


@dataclasses.dataclass
class ShortGroup:
    name: str
    dtype: str
    kind: str
    layers: List[Short]         # T = 0: a layer the call skips
    share_w: bool               # every layer reads the first layer's accumulator (one W, or one code matrix and its scales)

    def entries(self):
        return sum(cdiv(c.T, 64) for c in self.layers)

    def pairs(self):
        return cdiv(self.entries(), SK_MAXL)

    def cuts_inside(self):
        """Indices of the layers whose row blocks a launch-pair boundary falls strictly inside."""
        out, e0 = [], 0
        for i, c in enumerate(self.layers):
            e1 = e0 + cdiv(c.T, 64)
            if any(e0 < cut < e1 for cut in range(SK_MAXL, self.entries(), SK_MAXL)):
                out.append(i)
            e0 = e1
        return out


def ref_cost(c) -> float:
    """Multiply-adds of the float64 products the checks of a case form on the CPU (fuzz_plan.ref_cost for these case types): the
    skinny comparator for Rows; test_gpu_elementwise._check on a dense layer for Short, and the x W / dY W^T products of the
    tie-clearing passes where they run (T <= 129: four passes, two products each)."""
    if isinstance(c, Rows):
        return (2.0 * c.T * c.d_in * c.d_out if c.kind != "none" else 0.0) + 16.0 * c.T * (c.d_in + c.d_out) * 64
    if isinstance(c, ShortGroup):
        return sum(ref_cost(m) for m in c.layers)
    return 14.0 * c.T * (c.d_in + c.d_out) * 64 + (4.0 + (8.0 if c.T <= 129 else 0.0)) * c.T * c.d_in * c.d_out


class _Draw:
    def __init__(self, seed):
        self.g = random.Random(seed)
        self.n = 3000

    def settings(self, c, scales):
        g = self.g
        c.bias = g.random() < 0.6
        c.s = g.choice(scales)
        c.seed = self.n
        self.n += 1
        return c


def _last_range(g, col, cn, nc):
    """N columns whose last range of cn is in class `col`, nc ranges (one for "lt")."""
    if col == "lt":      # (from 24 up: a contraction of 8 or 16 leaves the tie-clearing step of the operands too few elements to move)
        return 8 * g.randint(3, cn // 8 - 1)
    return {"8": (nc - 1) * cn + 8, "cn-8": nc * cn - 8, "0": nc * cn}.get(col) or (nc - 1) * cn + 8 * g.randint(2, cn // 8 - 2)


def _fwd_tail_values(g, tail, ks, step):
    if tail == "kgroup":
        return [step]
    if tail == "full":
        return [ks]
    lo = 512 if tail == ">512" else step
    vals = [t for t in range(lo + step, ks, step) if t % 128]
    return g.sample(vals, min(len(vals), 6))


def _bwd_tail_values(g, tail, ks):
    if tail == "kgroup":
        return [8]
    if tail == "full":
        return [ks]
    vals = [t for t in range(16, ks, 8) if bwd_tail_class(t, 1, ks) == tail]
    return g.sample(vals, min(len(vals), 6))


def _contraction(g, lo, hi, ks, tails, big_s):
    """K = (S - 1) ks + tail inside [lo, hi], with more than 16 slabs for big_s: one of the smallest quarter of the candidates."""
    cands = sorted({(S - 1) * ks + t for t in tails for S in range(max(cdiv(lo, ks) - 1, 17 if big_s else 1), hi // ks + 2)
                    if lo <= (S - 1) * ks + t <= hi})
    return g.choice(cands[:max(len(cands) // 4, 1)]) if cands else None


def _band(want, ks, kq, ks_max, step):
    """[lo, hi] of the contraction lengths that plan slabs of ks at `want` slabs' worth of workgroups."""
    if ks == kq:
        return step, want * kq
    if ks == ks_max:
        return want * (ks - kq) + 1, 1 << 30
    return want * (ks - kq) + 1, want * ks


# ---- rows: sow_forward_skinny_rows -----------------------------------------------------------------------------------------------------
# per kind with an accumulator: (T <= 48, slab length, tail class, column class, more than 16 slabs, the clamp binds).  One case at
# each length from 256 up in either range of T (matrices of 3 M to 25 M elements), the rest at 128
_ROWS_DENSE = [(True, 256, "full", "other", False, False), (True, 384, "kgroup", "8", False, False), (True, 512, "partial", "cn-8", False, False),
               (True, 640, ">512", "0", False, False), (True, 768, ">512", "other", False, False),
               (False, 256, "kgroup", "cn-8", False, False), (False, 384, "partial", "0", False, False), (False, 512, "full", "8", False, True),
               (True, 128, "kgroup", "lt", False, False), (True, 128, "partial", "8", True, False), (True, 128, "full", "cn-8", False, False),
               (True, 128, "partial", "0", False, False), (False, 128, "kgroup", "0", False, False), (False, 128, "partial", "other", True, False),
               (False, 128, "full", "lt", False, False), (False, 128, "partial", "8", False, False)]
_ROWS_NONE = [(True, 128, "kgroup", "8", False, False), (False, 128, "partial", "cn-8", False, False), (True, 128, "full", "0", False, False),
              (False, 128, "partial", "lt", True, False), (True, 256, "partial", "lt", False, False), (False, 384, "full", "other", False, False),
              (False, 512, "kgroup", "lt", False, True), (True, 768, ">512", "8", False, False)]


def _rows_shape(g, kind, low, ks, tail, col, big_s, clamp):
    cn, step = sk_cn(kind), sk_step(kind)
    total = ROWS_WANT8 if kind in CODES else ROWS_WANT
    ks_max = KS_MAX48 if low else KS_MAX64
    for _ in range(200):
        if kind == "none":
            d_out, want = _last_range(g, col, 64, g.randint(2, 6)), 32
        else:
            nc = g.randint(2, 12) if ks == 128 else g.randint(total // 16, total // 4)
            d_out = _last_range(g, col, cn, nc)
            want = cdiv(total, cdiv(d_out, cn))
        lo, hi = _band(want, ks, 128, ks_max, step)
        if clamp:                     # a d_in that plans more than 512 at T <= 48
            lo = want * 512 + 1
        hi = min(hi, 8192 if ks == 128 else lo + 4 * ks)
        d_in = _contraction(g, lo, hi, ks, _fwd_tail_values(g, tail, ks, step), big_s)
        if d_in:
            return d_in, d_out
    raise AssertionError(f"no rows shape for {kind} KS {ks} tail {tail} col {col}")


def _rows_name(c: Rows):
    S, ks, _ = c.plan()
    return f"rows_{c.kind}_{c.dtype}_T{c.T}_{c.d_in}x{c.d_out}_r{c.r}_KS{ks}x{S}" + ("_bias" if c.bias else "") + ("_f32" if c.f32 else "")


def _ranks(g, n, odd):
    """n ranks uniform over 1 .. 64 with every value of SK_R_EDGES once more; drawn again until `odd` of them are odd."""
    while True:
        rs = [g.randint(1, 64) for _ in range(n)]
        for v, i in zip(SK_R_EDGES, g.sample(range(n), len(SK_R_EDGES))):
            rs[i] = v
        if sum(r % 2 for r in rs) >= odd:
            return rs


def _rows(d: _Draw) -> List[Rows]:
    g = d.g
    specs = [(kind,) + sp for kind in KINDS[:3] for sp in _ROWS_DENSE] + [("none",) + sp for sp in _ROWS_NONE]
    n = len(specs)
    rs = _ranks(g, n, cdiv(n, 3))
    Ts = [g.randint(33, 48) if sp[1] else g.randint(49, 64) for sp in specs]
    for kind in KINDS:                 # every edge of T once per kind, on a case of its side of 48
        for low, edges in ((True, ROWS_T_EDGES[:3]), (False, ROWS_T_EDGES[3:])):
            mine = [j for j, sp in enumerate(specs) if sp[0] == kind and sp[1] == low]
            for v, j in zip(edges, g.sample(mine, 3)):
                Ts[j] = v
    out = []
    for j, (kind, low, ks, tail, col, big_s, clamp) in enumerate(specs):
        d_in, d_out = _rows_shape(g, kind, low, ks, tail, col, big_s, clamp)
        c = d.settings(Rows("", "bf16" if j % 2 == 0 else "f16", kind, Ts[j], d_in, d_out, rs[j], True, 1.0, j % 3 == 0, 0),
                       SCALES + (1.0 / rs[j],))
        c.name = _rows_name(c)
        assert c.plan()[1] == ks and tail in c.tails() and c.col() == col and (c.plan()[0] > 16 or not big_s), c.name
        out.append(c)
    return out


# ---- short, short_codes ------------------------------------------------------------------------------------------------------------------
# (led direction, slab length, tail class, more than 16 slabs): every length of either direction with every tail class of it
_SHORT_SPECS = ([("f", ks, t, False) for ks in (128, 256, 384, 512) for t in FWD_TAILS[:3]]
                + [("b", ks, t, False) for ks in (256, 512) for t in BWD_TAILS]
                + [("f", 128, "partial", True), ("b", 256, "pair+", True), ("f", 128, "full", False), ("b", 256, "idle", False)])


def _short_Ts(g):
    """SHORT_T_FIXED once each, then ten of 3 .. 15 row blocks whose last block holds 16, 17, 32, 33 or 47 rows: every block-count
    class and every count of LAST_ROWS at least twice."""
    return list(SHORT_T_FIXED) + [64 * g.randint(2, 14) + e for e in (16, 17, 32, 33, 47) for _ in range(2)]


def _short_shape(g, kind, T, led, ks, tail, col, big_s):
    """(d_in, d_out): the led direction plans slabs of ks with the last one in class `tail`, its last column range in class `col`."""
    nblk = cdiv(T, 64)
    for _ in range(400):
        if led == "f":
            cn, total, kq, step = sk_cn(kind), (SHORT_WANT8 if kind in CODES else SHORT_WANT), KQ_FWD, sk_step(kind)
            N = _last_range(g, col, cn, g.randint(2, 5))
            tails = _fwd_tail_values(g, tail, ks, step)
        else:
            cn, total, kq, step = 64, SHORT_WANT, KQ_BWD, 8
            if kind == "mxfp4":
                N = 32 if col == "=32" else 64 * g.randint(1, 5) + int(col)
            else:
                N = _last_range(g, col, 64, g.randint(2, 5))
            tails = _bwd_tail_values(g, tail, ks)
        want = cdiv(total, cdiv(N, cn) * nblk)
        lo, hi = _band(want, ks, kq, KS_MAX64, step)
        hi = min(hi, max(8192, 24 * ks) if ks == kq else lo + 4 * ks)
        K = _contraction(g, lo, hi, ks, tails, big_s)
        if K:
            return (K, N) if led == "f" else (N, K)
    raise AssertionError(f"no short shape for {kind} T {T} {led} KS {ks} tail {tail} col {col}")


def _short_name(c: Short, tag):
    (sf, kf, _), (sb, kb, _) = c.fwd(), c.bwd()
    return f"{tag}_{c.kind}_{c.dtype}_T{c.T}_{c.d_in}x{c.d_out}_r{c.r}_KS{kf}x{sf}_KS{kb}x{sb}" + ("_bias" if c.bias else "")


def _short(d: _Draw, codes: bool) -> List[Short]:
    g = d.g
    specs = list(_SHORT_SPECS)
    n = len(specs)
    Ts = sorted(_short_Ts(g), reverse=True)
    assert len(Ts) == n
    # the cases whose led direction leaves the shortest slab take the longest batches: the plan counts the row blocks, and W stays small
    heavy = [j for j, sp in enumerate(specs) if sp[1] > (KQ_FWD if sp[0] == "f" else KQ_BWD)]
    light = [j for j in range(n) if j not in heavy]
    g.shuffle(heavy)
    g.shuffle(light)
    T_of = dict(zip(heavy + light, Ts))
    rs = _ranks(g, n, cdiv(n, 3))
    turn, n16 = {}, {}
    out = []
    for j, (led, ks, tail, big_s) in enumerate(specs):
        if codes:      # the formats in turn such that each meets every slab length and every tail class of either direction
            tails = FWD_TAILS if led == "f" else BWD_TAILS
            kind = CODES[((ks // (KQ_FWD if led == "f" else KQ_BWD) - 1) + tails.index(tail) + (j >= 22)) % 2]
        else:
            kind = "dense"
        cols = COLS_FP4_BWD if (kind == "mxfp4" and led == "b") else COLS
        k = turn.get((kind, led), 0)
        turn[(kind, led)] = k + 1
        d_in, d_out = _short_shape(g, kind, T_of[j], led, ks, tail, cols[k % len(cols)], big_s)
        # f16 where the tie-clearing step of the operands does not run (T > 129) or has few rows to clear (T <= 17), two in three of
        # those per format; bf16 between: there an f16 column of h over a narrow or a very long contraction often stays within the
        # fp32 noise of a midpoint in some row after every move (test_gpu_short_rows.TIES_MAX_T), and such a shape would have to go
        n16[kind] = n16.get(kind, 0) + (T_of[j] > 129 or T_of[j] <= 17)
        f16 = (T_of[j] > 129 or T_of[j] <= 17) and n16[kind] % 3 != 0
        c = d.settings(Short("", "f16" if f16 else "bf16", kind, T_of[j], d_in, d_out, rs[j], True, 1.0, 0, led), SCALES)
        c.name = _short_name(c, "codes" if codes else "short")
        S, k_, _ = c.fwd() if led == "f" else c.bwd()
        assert k_ == ks and (tail in c.fwd_tails() if led == "f" else c.bwd_tail() == tail) and (S > 16 or not big_s), c.name
        out.append(c)
    return out


# ---- short_groups ------------------------------------------------------------------------------------------------------------------------
# (format, dtype, row counts, one accumulator for all).  Row blocks: 10 + 16 + 8 = 34 entries in three launch pairs, the cuts inside the
# middle and the last layer; 3 + 0 + 5 + 9 + 1 = 18 in two, a T = 0 layer between live ones and the cut inside the fourth layer; sixteen
# layers of one to four blocks; two layers on one W.  The same on codes: 15 + 10 + 8 = 33; 2 + 4 + 0 + 11 + 1 = 18
_GROUP_SPECS = [("dense", "bf16", (600, 1000, 500), False), ("dense", "f16", (130, 0, 300, 520, 64), False), ("dense", "bf16", 16, False),
                ("dense", "bf16", (100, 129), True),
                ("e4m3", "bf16", (900, 600, 500), False), ("e4m3", "f16", (65, 200, 0, 700, 17), False), ("mxfp4", "bf16", 16, False),
                ("mxfp4", "bf16", (100, 129), True)]


def _short_groups(d: _Draw) -> List[ShortGroup]:
    g = d.g
    out = []
    for i, (kind, dt, Ts, share) in enumerate(_GROUP_SPECS):
        if Ts == 16:
            Ts = [g.randint(1, 64) for _ in range(12)] + [g.randint(65, 256) for _ in range(4)]
            g.shuffle(Ts)
        step = sk_step(kind)
        layers = []
        for j, T in enumerate(Ts):
            d_in, d_out = (layers[0].d_in, layers[0].d_out) if share and layers else (step * g.randint(64 // step, 320 // step), 8 * g.randint(8, 40))
            c = d.settings(Short("", dt, kind, T, d_in, d_out, g.randint(1, 64), True, 1.0, 0), SCALES)
            c.name = _short_name(c, f"sg{i}.{j}") if T else f"sg{i}.{j}_{kind}_{dt}_T0_{d_in}x{d_out}_r{c.r}"
            layers.append(c)
        out.append(ShortGroup(f"shortgroup{i}_{kind}_{dt}_n{len(layers)}_e{sum(cdiv(T, 64) for T in Ts)}" + ("_oneW" if share else ""),
                              dt, kind, layers, share))
    return out


@dataclasses.dataclass
class Plan:
    rows: List[Rows]
    short: List[Short]
    short_codes: List[Short]
    short_groups: List[ShortGroup]


def plan(seed: int = SEED) -> Plan:
    d = _Draw(seed)
    return Plan(_rows(d), _short(d, False), _short(d, True), _short_groups(d))
