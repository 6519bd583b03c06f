"""CPU tests of the blocked Householder QR (sow_amd/csrc/qr_blocked.hip, sow_qr_thin past 64 factored columns):

1. the NO_BLOCKED_QR switch exists and round-trips through sow_set_switch / sow_get_switch / _lib.switch;
2. sow_qr_workspace_bytes is a pure function of the shape (the same with the switch off and on) and unchanged where the
   blocked route never runs (kc <= 64);
3. a float32 numpy emulation of the compact-WY algorithm in the kernels' structure -- unblocked panel on the rows j0.. of a
   block (slarfg signs and taus of qr_panel.hpp), T by the columnwise recurrence T[:j, j] = -tau_j T[:j, :j] V[:, :j]^T v_j,
   trailing update C <- (I - V T^T V^T) C, Q from the blocks in reverse order applied to I[:, :k], R tail Q^T W -- passes
   step_numerics.check_qr with the committed bound C_QR for block widths 32 and 64: the bound has room for the blocked
   operation order, whatever the kernel does.

No GPU work is attempted.  QR_BLOCKED_CASES is shared with tests/test_gpu_qr_blocked.py."""
import numpy as np
import pytest
import torch

from step_numerics import check_qr
from sow_amd import _lib

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

QR_BLOCKED_CASES = [  # (m, n, k, in, out, need_r, extra ld, scale)
    (200, 200, 200, F32, F32, 1, 0, 1.0), (259, 130, 97, F32, F32, 1, 0, 1.0), (130, 259, 65, BF16, BF16, 1, 0, 1.0),
    (300, 70, 150, F16, F32, 1, 0, 1.0),          # complete mode: kc = 70 factored columns, 150 columns of Q
    (257, 96, 96, F32, F16, 1, 0, 1.0), (384, 384, 129, F32, F32, 1, 0, 1.0),
    (512, 256, 256, F32, F32, 1, 0, 1e-12), (512, 256, 256, BF16, F32, 1, 0, 1e12), (1001, 300, 600, F32, F32, 1, 0, 1.0),
    (384, 200, 160, BF16, F32, 0, 0, 1.0),        # Q only
    (321, 150, 131, F16, F32, 1, 5, 1.0),         # row pitch n + 5
]
RANK_DEFICIENT = ["zero_column", "repeated_column", "zero_columns_at_block_edge"]


def case_input(m, n, k, din, scale):
    return (torch.randn(m, n, generator=torch.Generator().manual_seed(m + n + k)) * scale).to(din)


def rank_deficient_input(kind):
    """300 x 120 (k = 80), as test_qr_thin_rank_deficient; the block-edge kind zeroes the last column of a block and the first
    of the next one for both block widths (31, 32 and 63, 64)."""
    W0 = torch.randn(300, 120, generator=torch.Generator().manual_seed(9))
    if kind == "zero_column":
        W0[:, 17] = 0
    elif kind == "repeated_column":
        W0[:, 40] = W0[:, 12]
    else:
        W0[:, [31, 32, 63, 64]] = 0
    return W0


# ---- switch and workspace -------------------------------------------------------------------------------------------------
def test_no_blocked_qr_switch_can_be_set_read_and_restored():
    lib = _lib.load()
    old = lib.sow_get_switch(b"NO_BLOCKED_QR")
    assert old in (-1, 0, 1), "the switch table has no NO_BLOCKED_QR"
    try:
        assert lib.sow_set_switch(b"NO_BLOCKED_QR", 1) == 0 and lib.sow_get_switch(b"NO_BLOCKED_QR") == 1
        assert lib.sow_set_switch(b"NO_BLOCKED_QR", 0) == 0 and lib.sow_get_switch(b"NO_BLOCKED_QR") == 0
        assert lib.sow_set_switch(b"NO_BLOCKED_QR", -1) == 0 and lib.sow_get_switch(b"NO_BLOCKED_QR") == -1
        with _lib.switch(NO_BLOCKED_QR=1):
            assert lib.sow_get_switch(b"NO_BLOCKED_QR") == 1
        assert lib.sow_get_switch(b"NO_BLOCKED_QR") == -1
        before = lib.sow_get_switch(b"NO_RAGGED_GEMM")      # a switch of its own
        with _lib.switch(NO_BLOCKED_QR=1):
            assert lib.sow_get_switch(b"NO_RAGGED_GEMM") == before
    finally:
        lib.sow_set_switch(b"NO_BLOCKED_QR", old)
    assert lib.sow_get_switch(b"NO_BLOCKED_QR") == old


def _al256(v):
    return (v + 255) // 256 * 256


def _one_workgroup_bytes(m, n, k, dt, need_r):
    """The query before the blocked route existed: panel [kc][m] and Q [k][m] in fp32, the fp32 copy of a 16-bit W tail, the
    fp32 R tail (the query assumes a 16-bit output), 256 bytes of alignment slack."""
    kc = min(k, m, n)
    b = _al256(kc * m * 4) + _al256(k * m * 4)
    if need_r and n > kc:
        b += (_al256(m * (n - kc) * 4) if dt != _lib.F32 else 0) + _al256(k * (n - kc) * 4)
    return b + 256


@pytest.mark.parametrize("m,n,k", [(1001, 300, 600), (2048, 5461, 2048), (259, 100, 50)])
def test_qr_workspace_is_a_function_of_the_shape(m, n, k):
    lib = _lib.load()
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        for need_r in (0, 1):
            with _lib.switch(NO_BLOCKED_QR=0):
                off = lib.sow_qr_workspace_bytes(m, n, k, dt, need_r)
            with _lib.switch(NO_BLOCKED_QR=1):
                on = lib.sow_qr_workspace_bytes(m, n, k, dt, need_r)
            assert off == on > 0, (m, n, k, dt, need_r, off, on)
            # the one-workgroup route's regions, plus one 32 x 32 fp32 tile of T per block of 32 columns when kc > 64
            kc = min(k, m, n)
            tiles = _al256(-(-kc // 32) * 32 * 32 * 4) if kc > 64 else 0
            assert off == _one_workgroup_bytes(m, n, k, dt, need_r) + tiles, (m, n, k, dt, need_r, off, tiles)


def test_qr_workspace_of_wide_panels_holds_the_t_tiles():
    """Literals: 1001 x 300, k = 600 factors 300 columns in 10 blocks (3604224 + 10 * 4096 bytes); 200 x 200 in 7 blocks
    (320256 + 7 * 4096); 2048 x 5461, k = 2048 in 64 blocks (61513984 + 64 * 4096 with R, fp32 input)."""
    lib = _lib.load()
    assert lib.sow_qr_workspace_bytes(1001, 300, 600, _lib.F32, 1) == 3645184
    assert lib.sow_qr_workspace_bytes(200, 200, 200, _lib.F32, 1) == 348928
    assert lib.sow_qr_workspace_bytes(2048, 5461, 2048, _lib.F32, 1) == 61776128


def test_qr_workspace_of_a_narrow_panel_is_unchanged():
    """259 x 100, k = 50 never takes the blocked route: the byte counts of the library before the blocked route existed."""
    lib = _lib.load()
    assert lib.sow_qr_workspace_bytes(259, 100, 50, _lib.F32, 0) == 104192
    assert lib.sow_qr_workspace_bytes(259, 100, 50, _lib.F32, 1) == 114432
    assert lib.sow_qr_workspace_bytes(259, 100, 50, _lib.BF16, 1) == 166400


# ---- float32 emulation ----------------------------------------------------------------------------------------------------
f32 = np.float32


def _panel(P, j0, jb):
    """Unblocked Householder on columns j0 .. j0 + jb of P, rows j0..; returns taus.  In place: R on and above the diagonal,
    the reflectors (v[0] = 1 implicit) below."""
    taus = np.zeros(jb, f32)
    for j in range(jb):
        c = j0 + j
        x = P[c + 1:, c]
        x2 = f32(np.sum(x * x, dtype=f32))
        alpha = P[c, c]
        tau = scale = f32(0)
        if x2 != 0:
            nrm = np.sqrt(f32(alpha * alpha + x2))
            beta = -nrm if alpha >= 0 else nrm
            tau = f32((beta - alpha) / beta)
            scale = f32(f32(1) / (alpha - beta))
            P[c, c] = beta
        taus[j] = tau
        P[c + 1:, c] = x * scale
        if tau != 0 and j + 1 < jb:
            v = np.concatenate([np.ones(1, f32), P[c + 1:, c]])
            blk = P[c:, c + 1:j0 + jb]
            d = (v @ blk).astype(f32) * tau
            blk -= np.outer(v, d).astype(f32)
    return taus


def _unit_lower(P, j0, jb):
    V = np.tril(P[j0:, j0:j0 + jb], -1).astype(f32)
    V[np.arange(jb), np.arange(jb)] = 1
    return V


def _form_t(V, taus):
    jb = len(taus)
    G = (V.T @ V).astype(f32)
    T = np.zeros((jb, jb), f32)
    for j in range(jb):
        T[j, j] = taus[j]
        if j and taus[j] != 0:
            T[:j, j] = -taus[j] * (T[:j, :j] @ G[:j, j]).astype(f32)
    return T


def blocked_qr_f32(W, k, nb):
    """Q[:, :k], R[:k, :] (float32 numpy) of the compact-WY factorisation of W (float32 [m, n]) by blocks of nb columns."""
    m, n = W.shape
    kc = min(k, m, n)
    P = W[:, :kc].astype(f32).copy()
    blocks = []
    for j0 in range(0, kc, nb):
        jb = min(nb, kc - j0)
        taus = _panel(P, j0, jb)
        V = _unit_lower(P, j0, jb)
        T = _form_t(V, taus)
        assert np.isfinite(T).all()
        blocks.append((j0, V, T))
        if j0 + jb < kc:
            C = P[j0:, j0 + jb:]
            C -= (V @ (T.T @ (V.T @ C).astype(f32)).astype(f32)).astype(f32)
    Q = np.eye(m, k, dtype=f32)
    for j0, V, T in reversed(blocks):
        C = Q[j0:, j0:]
        C -= (V @ (T @ (V.T @ C).astype(f32)).astype(f32)).astype(f32)
    R = np.zeros((k, n), f32)
    R[:kc, :kc] = np.triu(P[:kc, :kc])
    if n > kc:
        R[:, kc:] = (Q.T @ W[:, kc:].astype(f32)).astype(f32)
    return Q, R


def _check_emulation(W0, k, dout, need_r, nb, name, against_lapack=True):
    Q, R = blocked_qr_f32(W0.float().numpy(), k, nb)
    Q, R = torch.from_numpy(Q).to(dout), torch.from_numpy(R).to(dout)
    st = check_qr(W0, Q, R if need_r else None, k, dout, name=name, against_lapack=against_lapack)
    print(f"{name} nb={nb}: " + ", ".join(f"{key} {s['worst']:.3g}" for key, s in st.items()))
    return st


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("m,n,k,din,dout,need_r,extra_ld,scale", QR_BLOCKED_CASES)
def test_blocked_emulation_passes_check_qr(m, n, k, din, dout, need_r, extra_ld, scale, nb):
    _check_emulation(case_input(m, n, k, din, scale), k, dout, need_r, nb, f"emulated qr {m}x{n} k={k}")


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("kind", RANK_DEFICIENT)
def test_blocked_emulation_rank_deficient(kind, nb):
    _check_emulation(rank_deficient_input(kind), 80, F32, 1, nb, f"emulated qr {kind}", against_lapack=False)


def test_t_of_a_zero_column_is_a_zero_column():
    """tau = 0 (H = I) gives a zero column of T and no NaN, and I - V T V^T is still the product of the reflectors."""
    W = rank_deficient_input("zero_columns_at_block_edge").numpy()[:, :40].astype(f32)
    P = W.copy()
    taus = _panel(P, 0, 40)
    assert taus[31] == 0 and taus[32] == 0
    V = _unit_lower(P, 0, 40)
    T = _form_t(V, taus)
    assert np.isfinite(T).all() and not T[:, 31].any() and not T[:, 32].any()
    H = np.eye(300)
    for j in range(40):
        v = V[:, j].astype(np.float64)
        H = H @ (np.eye(300) - float(taus[j]) * np.outer(v, v))
    WY = np.eye(300) - V.astype(np.float64) @ T.astype(np.float64) @ V.T.astype(np.float64)
    assert np.abs(H - WY).max() < 300 * 2.0 ** -24
