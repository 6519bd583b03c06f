"""CPU tests of the shared-input sibling path (sow_forward_shared / sow_backward_shared, group_siblings(shared_input=True)):
the C-ABI surface, the host-side argument checks that run before anything is launched, and the module plumbing."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from sow_amd import SoWLinear, _lib, group_siblings, ops, ungroup_siblings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = 1


def test_shared_entry_points_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sow_amd.h")).read(), flags=re.S)
    for name in ("sow_forward_shared", "sow_backward_shared"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.SIGNATURES["sow_forward_shared"][1][0] is ctypes.POINTER(_lib.LayerArgs)
    assert len(_lib.SIGNATURES["sow_backward_shared"][1]) == 5
    assert _lib.load().sow_get_switch(b"NO_SHARED_X") in (-1, 0, 1)   # a known switch name (unknown: SOW_ERR_UNSUPPORTED)


def _fake_layers(n, T=32768, d_in=512, d_outs=(512, 512, 512)):
    """Layer descriptors whose pointers are never dereferenced: the calls below must return from host checks."""
    arr = (_lib.LayerArgs * n)()
    for i in range(n):
        a = arr[i]
        base = 0x10000000 * (i + 1)
        a.x, a.A, a.B, a.y, a.h_save = 0x1000000, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000
        a.dy, a.dx, a.dA, a.dB, a.workspace = base + 0x5000, 0x2000000, base + 0x6000, base + 0x7000, base + 0x8000
        a.T, a.d_in, a.d_out, a.r_live, a.scale, a.workspace_bytes = T, d_in, d_outs[i], 50, 0.5, 1 << 30
    return arr


def test_shared_host_checks_launch_nothing():
    lib = _lib.load()
    arr = _fake_layers(3)
    arr[1].x = 0x1000100                                      # a different input: not one sibling set
    assert lib.sow_forward_shared(arr, 3, BF16, None) == _lib.ERR_SHAPE
    assert lib.sow_backward_shared(arr, 3, BF16, 1, None) == _lib.ERR_SHAPE
    arr = _fake_layers(3)
    arr[2].dx = 0x2000100                                     # a second dX: the set has one
    assert lib.sow_backward_shared(arr, 3, BF16, 1, None) == _lib.ERR_SHAPE
    arr[2].dx = None                                          # NULL: takes layers[0].dx
    arr[1].d_in = 256
    assert lib.sow_backward_shared(arr, 3, BF16, 1, None) == _lib.ERR_SHAPE
    assert lib.sow_forward_shared(arr, 0, BF16, None) == _lib.ERR_SHAPE
    assert lib.sow_forward_shared(_fake_layers(3), 3, 7, None) == -3               # SOW_ERR_DTYPE
    arr = _fake_layers(3)
    arr[0].A = None
    assert lib.sow_forward_shared(arr, 3, BF16, None) == -1                       # SOW_ERR_NULL
    with _lib.switch(NO_SHARED_X=1):
        assert lib.sow_forward_shared(_fake_layers(3), 3, BF16, None) == _lib.ERR_UNSUPPORTED
        assert lib.sow_backward_shared(_fake_layers(3), 3, BF16, 1, None) == _lib.ERR_UNSUPPORTED
    # outside the admitted set: short T, a rank above 64, fp32, SOW_PARAM_F32, more than 4 siblings
    assert lib.sow_forward_shared(_fake_layers(3, T=8192), 3, BF16, None) == _lib.ERR_UNSUPPORTED
    arr = _fake_layers(3)
    arr[1].r_live = 100
    assert lib.sow_forward_shared(arr, 3, BF16, None) == _lib.ERR_UNSUPPORTED
    assert lib.sow_forward_shared(_fake_layers(3), 3, 0, None) == _lib.ERR_UNSUPPORTED
    assert lib.sow_forward_shared(_fake_layers(3), 3, BF16 | 0x100, None) == _lib.ERR_UNSUPPORTED
    assert lib.sow_backward_shared(_fake_layers(3), 3, BF16 | 0x100, 2, None) == _lib.ERR_UNSUPPORTED   # weights only too
    arr = _fake_layers(3)
    arr[0].acc_kind, arr[0].acc_down = 1, 0x3000000       # dense accumulator
    assert lib.sow_backward_shared(arr, 3, BF16, 1, None) == _lib.ERR_UNSUPPORTED
    big = (_lib.LayerArgs * 5)(*([_fake_layers(1)[0]] * 5))
    assert lib.sow_forward_shared(big, 5, BF16, None) == _lib.ERR_UNSUPPORTED


class _Attn(nn.Module):
    def __init__(self, d=32, r=4):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = (SoWLinear(d, d, rank=r, init_method="normal") for _ in range(3))

    def forward(self, x):
        return self.q_proj(x) + self.k_proj(x) + self.v_proj(x)


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = _Attn()
        self.mlp = nn.Module()
        self.mlp.gate_proj, self.mlp.up_proj = SoWLinear(32, 48, rank=4, init_method="normal"), SoWLinear(32, 48, rank=4, init_method="normal")


def test_group_siblings_plumbs_shared_input():
    model = _Block()
    assert group_siblings(model) == 2
    assert all(not m._sibling_group.shared_input for m in (model.self_attn.q_proj, model.mlp.up_proj))
    ungroup_siblings(model)
    assert group_siblings(model, shared_input=True) == 2
    q = model.self_attn.q_proj
    assert q._sibling_group.shared_input and q._sibling_group is model.self_attn.v_proj._sibling_group
    assert model.mlp.gate_proj._sibling_group.shared_input
    ungroup_siblings(model)
    assert not hasattr(q, "_sibling_group")


def test_shared_input_refuses_cpu_tensors():
    model = _Block()
    group_siblings(model, shared_input=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.self_attn(torch.randn(2, 5, 32))
    x = torch.randn(16, 32)
    A, B = torch.randn(32, 4), torch.randn(4, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.SharedInputGroup([ops.LayerCall(x, A, B, forward_only=True), ops.LayerCall(x, A, B, forward_only=True)])
