"""CPU: the host side of SOW_FUSE_ACC_DEEP -- the flag constant, the Python mirror of the admitted set, the LDS plan, the
permission plumbing of ops.LayerCall / LayerGroup, and the workspace queries, which are pure host functions."""
import os
import re

import pytest
import torch

from sow_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LR, DENSE, NONE = _lib.ACC_LOWRANK, _lib.ACC_DENSE, _lib.ACC_NONE
DEEP, FUSE = _lib.FUSE_ACC_DEEP, _lib.FUSE_ACC


def test_flag_constant_matches_the_header():
    text = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    m = re.search(r"#define\s+SOW_FUSE_ACC_DEEP\s+(0x[0-9a-fA-F]+)", text)
    assert m and int(m.group(1), 16) == DEEP == 0x400
    assert DEEP & (_lib.PARAM_F32 | FUSE | 0xFF) == 0          # a bit of its own, next to the dtype codes and the other flags
    assert "NO_DEEP_ACC" in text


# (d_in, d_out, r, r_acc, kind, dtype, param_f32) -> admitted
ADMITS = [
    ((512, 512, 58, 200, LR, BF16, False), True),       # total 258
    ((512, 1376, 50, 450, LR, BF16, False), True),
    ((1376, 512, 50, 500, LR, F16, False), True),
    ((136, 264, 64, 256, LR, BF16, False), True),       # total 320, r = 64
    ((1024, 1024, 50, 910, LR, BF16, False), True),     # total exactly 960
    ((8, 24, 2, 256, LR, BF16, False), True),
    ((768, 768, 8, 504, LR, BF16, False), True),
    ((512, 512, 56, 200, LR, BF16, False), False),      # total 256: the set of SOW_FUSE_ACC
    ((512, 512, 50, 50, LR, BF16, False), False),
    ((1024, 1024, 52, 910, LR, BF16, False), False),    # total 962
    ((512, 512, 66, 250, LR, BF16, False), False),      # r_live > 64
    ((512, 512, 50, 251, LR, BF16, False), False),      # odd r_acc
    ((512, 512, 49, 250, LR, BF16, False), False),      # odd r_live
    ((512, 260, 50, 250, LR, BF16, False), False),      # d_out % 8
    ((76, 264, 50, 250, LR, BF16, False), False),       # d_in % 8
    ((512, 512, 50, 0, NONE, BF16, False), False),
    ((512, 512, 50, 0, DENSE, BF16, False), False),
    ((512, 512, 50, 250, LR, F32, False), False),
    ((512, 512, 50, 250, LR, BF16, True), False),       # SOW_PARAM_F32: the permission is ignored
]


@pytest.mark.parametrize("args,want", ADMITS)
def test_deep_acc_admits(args, want):
    assert ops.deep_acc_admits(*args) is want
    assert not (want and ops.fused_acc_admits(*args))    # disjoint by the total


@pytest.mark.parametrize("args,want", ADMITS)
def test_library_plan_agrees_with_the_python_predicate(args, want):
    """The flagged workspace query is > 0 and >= the plain one on the admitted set (the forward query becomes the same
    figure), and equals the plain one outside -- the C predicate and its Python mirror agree."""
    lib = _lib.load()
    d_in, d_out, r, r_acc, kind, dtype, pf = args
    dt = ops._DT[dtype] | (_lib.PARAM_F32 if pf else 0)
    T = 300
    plain = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt)
    flagged = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | DEEP)
    fwd = lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | DEEP)
    both = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | DEEP | FUSE)
    assert plain > 0
    if want:
        assert flagged > 0 and flagged >= plain and fwd == flagged == both
        if r_acc > 256:      # the unflagged path packs nothing past 256 columns: the flagged plan is strictly larger
            assert flagged > plain
    else:
        assert flagged == plain
        assert fwd == lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt)
        assert both == lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt | FUSE)


def test_flagged_plan_keeps_every_unflagged_offset():
    """The flagged plan is the unflagged one with a wider last region: the difference is the difference of the pack sizes
    (r_pad rows of d_in and of d_out, two bytes each, each image rounded to 256 bytes)."""
    lib = _lib.load()
    T, d_in, d_out, r, r_acc = 300, 512, 1376, 50, 450     # unflagged: no wide region at all (r_acc > 256)
    plain = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, LR, _lib.BF16)
    flagged = lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, LR, _lib.BF16 | DEEP)
    r_pad = (r + r_acc + 63) // 64 * 64
    assert flagged - plain == r_pad * d_in * 2 + r_pad * d_out * 2


def test_lds_plan():
    assert ops.deep_acc_lds_bytes(960) == 160 * 1024 == ops.DEEP_ACC_MAX_LDS
    assert ops.deep_acc_lds_bytes(320) == 80 * 1024
    assert ops.deep_acc_lds_bytes(258) == ops.deep_acc_lds_bytes(320) and ops.deep_acc_lds_bytes(321) == 88 * 1024
    assert ops.deep_acc_lds_bytes(ops.DEEP_ACC_MAX_TOT + 2) > ops.DEEP_ACC_MAX_LDS


def test_switch_is_known_and_does_not_change_the_plan():
    lib = _lib.load()
    q = lambda: (lib.sow_workspace_bytes(300, 512, 264, 50, 300, LR, _lib.BF16 | DEEP),
                 lib.sow_forward_workspace_bytes(300, 512, 264, 50, 300, LR, _lib.BF16 | DEEP))
    before = q()
    assert lib.sow_get_switch(b"NO_DEEP_ACC") == -1
    with _lib.switch(NO_DEEP_ACC=1):
        assert lib.sow_get_switch(b"NO_DEEP_ACC") == 1
        assert q() == before
    assert q() == before and lib.sow_get_switch(b"NO_DEEP_ACC") == -1


def test_fuse_acc_alone_plans_as_before_on_total_258():
    lib = _lib.load()
    args = (193, 72, 264, 58, 200, LR)
    assert lib.sow_workspace_bytes(*args, _lib.BF16 | FUSE) == lib.sow_workspace_bytes(*args, _lib.BF16)
    assert lib.sow_forward_workspace_bytes(*args, _lib.BF16 | FUSE) == lib.sow_forward_workspace_bytes(*args, _lib.BF16)
    assert lib.sow_workspace_bytes(*args, _lib.BF16 | DEEP) > lib.sow_workspace_bytes(*args, _lib.BF16)
    # and the deep bit alone does nothing to the set of SOW_FUSE_ACC
    args = (193, 72, 264, 50, 50, LR)
    assert lib.sow_workspace_bytes(*args, _lib.BF16 | DEEP) == lib.sow_workspace_bytes(*args, _lib.BF16)
    assert lib.sow_workspace_bytes(*args, _lib.BF16 | DEEP | FUSE) == lib.sow_workspace_bytes(*args, _lib.BF16 | FUSE)


def test_other_entry_points_ignore_the_bit():
    lib = _lib.load()
    assert lib.sow_gemm_workspace_bytes(1024, 2048, 6144, 0, _lib.BF16 | DEEP) == lib.sow_gemm_workspace_bytes(1024, 2048, 6144, 0, _lib.BF16)
    assert lib.sow_qr_workspace_bytes(512, 264, 50, _lib.BF16 | DEEP, 1) == lib.sow_qr_workspace_bytes(512, 264, 50, _lib.BF16, 1)
    assert (lib.sow_forward_skinny_workspace_bytes(8, 512, 264, 50, DENSE, _lib.BF16 | DEEP)
            == lib.sow_forward_skinny_workspace_bytes(8, 512, 264, 50, DENSE, _lib.BF16) > 0)
    # the shared entry points take the bit as they take an unflagged dtype: an empty set is a shape error, not a dtype error
    assert lib.sow_forward_shared(None, 0, _lib.BF16 | DEEP, None) == lib.sow_forward_shared(None, 0, _lib.BF16, None) == -2
    assert lib.sow_backward_shared(None, 0, _lib.BF16 | DEEP, 1, None) == lib.sow_backward_shared(None, 0, _lib.BF16, 1, None) == -2
    # T = 0 calls return before anything is dereferenced: the bit is not a dtype error
    assert lib.sow_forward(None, None, None, None, None, None, None, None, 0, 512, 264, 50, 300, LR, 1.0, _lib.BF16 | DEEP, None, 0,
                           None) == 0
    assert lib.sow_forward(None, None, None, None, None, None, None, None, 0, 512, 264, 50, 300, LR, 1.0, 7 | DEEP, None, 0,
                           None) == -3


def test_call_dtype_carries_one_permission():
    x = torch.empty(4, 8, dtype=BF16)
    assert ops._call_dtype(x, False, fuse_acc=DEEP)[0] == _lib.BF16 | DEEP
    assert ops._call_dtype(x, False, fuse_acc=FUSE)[0] == ops._call_dtype(x, False, fuse_acc=True)[0] == _lib.BF16 | FUSE
    assert ops._call_dtype(x, False, fuse_acc=0)[0] == ops._call_dtype(x, False)[0] == _lib.BF16
    assert ops._call_dtype(x, True, fuse_acc=DEEP) == (_lib.BF16 | _lib.PARAM_F32, F32)     # ignored next to fp32 parameters
    assert ops._call_dtype(torch.empty(4, 8), False, fuse_acc=DEEP)[0] == _lib.F32          # ... and for fp32 tensors
    with pytest.raises(ValueError):
        ops._call_dtype(x, False, fuse_acc=FUSE | DEEP)     # one value per call


def test_layer_call_and_group_plumb_the_permission(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "_ws", lambda n, dev: torch.empty(max(int(n), 256), dtype=torch.uint8))
    monkeypatch.setattr(ops, "_workspace_bytes", lambda lib, *a: (seen.append(("bwd", a[-1])), 8192 if a[-1] & DEEP else 4096 if a[-1] & FUSE else 1024)[1])
    monkeypatch.setattr(ops, "_forward_workspace_bytes", lambda lib, *a: (seen.append(("fwd", a[-1])), 2048 if a[-1] & (DEEP | FUSE) else 0)[1])
    monkeypatch.setattr(_lib, "load", lambda: None)
    x = torch.zeros(16, 72, dtype=BF16)
    A, B = torch.zeros(72, 50, dtype=BF16), torch.zeros(50, 264, dtype=BF16)
    Q, R = torch.zeros(72, 300, dtype=BF16), torch.zeros(300, 264, dtype=BF16)
    monkeypatch.setattr(ops, "check_accumulator", lambda *a, **k: (LR, 300))
    deep = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=DEEP)
    assert deep.dtype == _lib.BF16 | DEEP and seen[-1] == ("bwd", deep.dtype) and deep.workspace.numel() == 8192
    c = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=DEEP, forward_only=True)
    assert seen[-1] == ("fwd", c.dtype) and c.args.workspace_bytes == 2048
    fused = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=True)
    plain = ops.LayerCall(x, A, B, acc_down=Q, acc_up=R)
    assert fused.dtype == _lib.BF16 | FUSE and plain.dtype == _lib.BF16
    # a caller's workspace of the unflagged plan is accepted (the library then runs the unflagged kernels), a smaller one is not
    ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=DEEP, workspace=torch.empty(1024, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.LayerCall(x, A, B, acc_down=Q, acc_up=R, fuse_acc=DEEP, workspace=torch.empty(512, dtype=torch.uint8))
    g = ops.LayerGroup([plain, deep, fused, deep])
    assert g.dtype == _lib.BF16 and g._perms == [0, DEEP, FUSE, DEEP]
    parts = g._by_permission()
    assert [(n, dt) for _, n, dt in parts] == [(1, _lib.BF16 | FUSE), (2, _lib.BF16 | DEEP), (1, _lib.BF16)]
    assert parts[1][0][0].workspace_bytes == deep.args.workspace_bytes
    assert ops.LayerGroup([deep, deep]).dtype == _lib.BF16 | DEEP and ops.LayerGroup([deep, deep])._fused is None
    launched = []
    monkeypatch.setattr(ops, "_launch", lambda dev, what, fn, arr, n, dt, *ph: launched.append((what, n, dt, *ph)))
    monkeypatch.setattr(_lib, "load", lambda: type("L", (), dict(sow_forward_group=None, sow_backward_group=None)))
    g.forward()
    g.backward(_lib.BWD_DATA | _lib.BWD_WEIGHTS_PARTIAL)
    Fd, Dd, P = _lib.BF16 | FUSE, _lib.BF16 | DEEP, _lib.BF16
    assert launched == [("sow_forward_group", 1, Fd), ("sow_forward_group", 2, Dd), ("sow_forward_group", 1, P),
                        ("sow_backward_group", 1, Fd, _lib.BWD_DATA), ("sow_backward_group", 2, Dd, _lib.BWD_DATA),
                        ("sow_backward_group", 1, P, _lib.BWD_DATA), ("sow_backward_group", 4, P, _lib.BWD_WEIGHTS_PARTIAL)]
    launched.clear()
    ops.LayerGroup([deep, deep]).backward()
    assert launched == [("sow_backward_group", 2, Dd, _lib.BWD_DATA | _lib.BWD_WEIGHTS)]


def test_module_permission_is_one_value(monkeypatch):
    monkeypatch.setattr(ops, "fused_acc_pays", lambda *a: True)
    monkeypatch.setattr(ops, "deep_acc_pays", lambda *a: True)
    assert ops.acc_permission(300, 512, 264, 50, 100, LR, BF16) == FUSE
    assert ops.acc_permission(300, 512, 264, 50, 300, LR, BF16) == DEEP
    assert ops.acc_permission(300, 512, 264, 50, 920, LR, BF16) == 0
    assert ops.acc_permission(300, 512, 264, 50, 300, LR, BF16, True) == 0
    monkeypatch.setattr(ops, "deep_acc_pays", lambda *a: False)
    assert ops.acc_permission(300, 512, 264, 50, 300, LR, BF16) == 0
    assert ops.acc_permission(300, 512, 264, 50, 100, LR, BF16) == FUSE


def test_nothing_unmeasured_is_on_by_default():
    """ops.deep_acc_pays is an envelope of the rows of profiles/deep_acc.txt: a minimum T and a maximum width per class of
    r_acc; the class that measured slower (r_acc a multiple of 8 past 256 columns) is off."""
    for d_in, d_out in ((512, 512), (512, 1376), (1376, 512), (1024, 1024)):
        for r_acc in (300, 450, 500, 900):
            assert ops.deep_acc_pays(32768, d_in, d_out, 50, r_acc)
        assert ops.deep_acc_pays(32768, d_in, d_out, 50, 250)
    assert ops.deep_acc_pays(16384, 512, 1376, 50, 450) and not ops.deep_acc_pays(16384, 512, 1376, 50, 250)
    for r_acc in (400, 504, 600):
        assert not ops.deep_acc_pays(32768, 768, 768, 50, r_acc)
    assert not ops.deep_acc_pays(ops.DEEP_ACC_MIN_T - 1, 512, 512, 50, 300)
    assert not ops.deep_acc_pays(1 << 40, ops.DEEP_ACC_MAX_D + 8, 512, 50, 300)
    assert not ops.deep_acc_pays(300, 512, 264, 50, 300)
