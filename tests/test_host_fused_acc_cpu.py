"""CPU: the host side of SOW_FUSE_ACC -- the flag constant, the Python mirror of the admitted set, the flag plumbing of
ops.LayerCall / LayerGroup, and the workspace queries, which are pure host functions."""
import os
import re

import pytest
import torch

from sow_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LR, DENSE, NONE = _lib.ACC_LOWRANK, _lib.ACC_DENSE, _lib.ACC_NONE


def test_flag_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    m = re.search(r"#define\s+SOW_FUSE_ACC\s+(0x[0-9a-fA-F]+)", text)
    assert m and int(m.group(1), 16) == _lib.FUSE_ACC == 0x200
    assert _lib.FUSE_ACC & (_lib.PARAM_F32 | 0xFF) == 0          # its own bit, next to the dtype codes and SOW_PARAM_F32
    assert "NO_FUSED_ACC" in text


# (d_in, d_out, r, r_acc, kind, dtype, param_f32) -> admitted
ADMITS = [
    ((512, 512, 50, 50, LR, BF16, False), True),
    ((512, 1376, 50, 200, LR, BF16, False), True),      # total 250
    ((520, 264, 64, 192, LR, F16, False), True),        # total exactly 256, r = 64
    ((8, 24, 2, 2, LR, BF16, False), True),
    ((768, 768, 8, 56, LR, BF16, False), True),
    ((512, 512, 58, 200, LR, BF16, False), False),      # total 258
    ((512, 512, 66, 50, LR, BF16, False), False),       # r_live > 64
    ((512, 512, 50, 208, LR, BF16, False), False),      # total 258 by r_acc
    ((512, 260, 50, 50, LR, BF16, False), False),       # d_out % 8
    ((76, 264, 50, 50, LR, BF16, False), False),        # d_in % 8
    ((512, 512, 49, 50, LR, BF16, False), False),       # odd r_live
    ((512, 512, 50, 51, LR, BF16, False), False),       # odd r_acc
    ((512, 512, 50, 0, NONE, BF16, False), False),
    ((512, 512, 50, 0, DENSE, BF16, False), False),
    ((512, 512, 50, 50, LR, F32, False), False),
    ((512, 512, 50, 50, LR, BF16, True), False),        # SOW_PARAM_F32: the permission is ignored
]


@pytest.mark.parametrize("args,want", ADMITS)
def test_fused_acc_admits(args, want):
    assert ops.fused_acc_admits(*args) is want


@pytest.mark.parametrize("args,want", ADMITS)
def test_library_plan_agrees_with_the_python_predicate(args, want):
    """The flagged workspace query grows exactly on the admitted set (never shrinks), and the forward query becomes
    non-zero there -- the C predicate and its Python mirror agree."""
    lib = _lib.load()
    d_in, d_out, r, r_acc, kind, dtype, pf = args
    dt = ops._DT[dtype] | (_lib.PARAM_F32 if pf else 0)
    T = 300
    plain = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt)
    flagged = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | _lib.FUSE_ACC)
    fwd = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | _lib.FUSE_ACC)
    if dtype == F32 and pf:
        return
    assert flagged >= plain
    if want:
        assert fwd == flagged > 0
        if r_acc <= 64:      # today's path packs nothing for a narrow accumulator: the flagged plan is strictly larger
            assert flagged > plain
    else:
        assert flagged == plain
        assert fwd == lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt)


def test_switch_does_not_change_the_plan():
    lib = _lib.load()
    q = lambda: (lib.sow_workspace_bytes(300, 512, 264, 50, 100, LR, _lib.BF16 | _lib.FUSE_ACC),
                 lib.sow_forward_workspace_bytes(300, 512, 264, 50, 100, LR, _lib.BF16 | _lib.FUSE_ACC))
    before = q()
    with _lib.switch(NO_FUSED_ACC=1):
        assert lib.sow_get_switch(b"NO_FUSED_ACC") == 1
        assert q() == before
    assert q() == before


def test_other_entry_points_ignore_the_flag():
    lib = _lib.load()
    F = _lib.FUSE_ACC
    assert lib.sow_gemm_workspace_bytes(1024, 2048, 6144, 0, _lib.BF16 | F) == lib.sow_gemm_workspace_bytes(1024, 2048, 6144, 0, _lib.BF16)
    assert lib.sow_qr_workspace_bytes(512, 264, 50, _lib.BF16 | F, 1) == lib.sow_qr_workspace_bytes(512, 264, 50, _lib.BF16, 1)
    assert (lib.sow_forward_skinny_workspace_bytes(8, 512, 264, 50, DENSE, _lib.BF16 | F)
            == lib.sow_forward_skinny_workspace_bytes(8, 512, 264, 50, DENSE, _lib.BF16) > 0)
    # T = 0 calls return before anything is dereferenced: the flag is not a dtype error any more
    assert lib.sow_forward(None, None, None, None, None, None, None, None, 0, 512, 264, 50, 100, LR, 1.0, _lib.BF16 | F, None, 0,
                           None) == 0
    assert lib.sow_forward(None, None, None, None, None, None, None, None, 0, 512, 264, 50, 100, LR, 1.0, 7 | F, None, 0,
                           None) == -3


def test_call_dtype_carries_the_flag():
    x = torch.empty(4, 8, dtype=BF16)
    assert ops._call_dtype(x, False, fuse_acc=True)[0] == _lib.BF16 | _lib.FUSE_ACC
    assert ops._call_dtype(x, False)[0] == _lib.BF16
    assert ops._call_dtype(x, True, fuse_acc=True) == (_lib.BF16 | _lib.PARAM_F32, F32)     # ignored next to fp32 parameters
    assert ops._call_dtype(torch.empty(4, 8), False, fuse_acc=True)[0] == _lib.F32          # ... and for fp32 tensors


def test_layer_call_plumbs_the_flag(monkeypatch):
    """LayerCall ORs the flag into the dtype it passes on, workspace queries included (the memo keys carry it)."""
    seen = []
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_ws", lambda n, dev: torch.empty(max(int(n), 256), dtype=torch.uint8))
    monkeypatch.setattr(ops, "_workspace_bytes", lambda lib, *a: (seen.append(("bwd", a[-1])), 4096 if a[-1] & _lib.FUSE_ACC else 1024)[1])
    monkeypatch.setattr(ops, "_forward_workspace_bytes", lambda lib, *a: (seen.append(("fwd", a[-1])), 2048 if a[-1] & _lib.FUSE_ACC else 0)[1])
    monkeypatch.setattr(_lib, "load", lambda: None)
    x = torch.zeros(16, 72, dtype=BF16)
    A, B = torch.zeros(72, 50, dtype=BF16), torch.zeros(50, 264, dtype=BF16)
    Q, R = torch.zeros(72, 50, dtype=BF16), torch.zeros(50, 264, dtype=BF16)
    monkeypatch.setattr(ops, "check_accumulator", lambda *a, **k: (LR, 50))
    c = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=True)
    assert c.dtype == _lib.BF16 | _lib.FUSE_ACC and seen[-1] == ("bwd", c.dtype) and c.workspace.numel() == 4096
    c = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=True, forward_only=True)
    assert seen[-1] == ("fwd", c.dtype) and c.args.workspace_bytes == 2048
    plain = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R)
    assert plain.dtype == _lib.BF16 and plain.workspace.numel() == 1024
    # a caller's workspace of the unflagged plan is accepted (the library then runs the two-pass kernels), a smaller one is not
    ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=True, workspace=torch.empty(1024, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=True, workspace=torch.empty(512, dtype=torch.uint8))
    # the permission belongs to each call: a mixed group issues its forward and its data gradient per kind
    g = ops.LayerGroup([plain, c, plain])
    assert g.dtype == _lib.BF16 and g._fused == [False, True, False]
    (fa, fn, fdt), (pa, pn, pdt) = g._by_permission()
    assert (fn, fdt, pn, pdt) == (1, _lib.BF16 | _lib.FUSE_ACC, 2, _lib.BF16)
    assert fa[0].workspace_bytes == c.args.workspace_bytes and pa[1].workspace_bytes == plain.args.workspace_bytes
    assert ops.LayerGroup([c, c]).dtype == _lib.BF16 | _lib.FUSE_ACC and ops.LayerGroup([c, c])._fused is None
    assert ops.LayerGroup([plain]).dtype == _lib.BF16 and ops.LayerGroup([plain])._fused is None
    launched = []
    monkeypatch.setattr(ops, "_launch", lambda dev, what, fn, arr, n, dt, *ph: launched.append((what, n, dt, *ph)))
    monkeypatch.setattr(_lib, "load", lambda: type("L", (), dict(sow_forward_group=None, sow_backward_group=None)))
    g.forward()
    g.backward(_lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL)
    g.backward(_lib.BWD_DATA)
    F, P = _lib.BF16 | _lib.FUSE_ACC, _lib.BF16
    assert launched == [("sow_forward_group", 1, F), ("sow_forward_group", 2, P),
                        ("sow_backward_group", 1, F, _lib.BWD_DATA), ("sow_backward_group", 2, P, _lib.BWD_DATA),
                        ("sow_backward_group", 3, P, _lib.BWD_WEIGHTS_PARTIAL),
                        ("sow_backward_group", 1, F, _lib.BWD_DATA), ("sow_backward_group", 2, P, _lib.BWD_DATA)]
    monkeypatch.setattr(_lib, "load", lambda: None)
    f16 = ops.LayerCall(x.half(), A.half(), B.half(), acc_down=Q.half(), acc_up=R.half())
    with pytest.raises(ValueError):
        ops.LayerGroup([plain, f16])


def test_pays_is_the_measured_envelope():
    """profiles/lowrank_acc.txt: T = 32768, widths up to 1376.  Nothing outside it is switched on."""
    for d_in, d_out in ((512, 512), (512, 1376), (1376, 512), (768, 768)):
        assert ops.fused_acc_pays(32768, d_in, d_out, 50, 100)
    assert not ops.fused_acc_pays(32767, 512, 512, 50, 100)
    assert not ops.fused_acc_pays(300, 512, 264, 50, 100)
    assert not ops.fused_acc_pays(32768, 2048, 2048, 50, 100) and not ops.fused_acc_pays(32768, 512, 1384, 50, 100)


def test_module_default_follows_admits_and_pays(monkeypatch):
    monkeypatch.setattr(ops, "fused_acc_pays", lambda *a: True)
    assert ops.fuse_acc_default(300, 512, 264, 50, 100, LR, BF16) is True
    assert ops.fuse_acc_default(300, 512, 260, 50, 100, LR, BF16) is False
    monkeypatch.setattr(ops, "fused_acc_pays", lambda *a: False)
    assert ops.fuse_acc_default(300, 512, 264, 50, 100, LR, BF16) is False
