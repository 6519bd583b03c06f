"""CPU tests of the float16 surface of the C ABI and of the host wrappers (no GPU compute)."""
import ctypes
import os
import re

import torch

from conftest import ROOT


def test_f16_dtype_code_matches_header():
    from sow_amd import _lib
    header = open(os.path.join(ROOT, "include", "sow_amd.h")).read()
    m = re.search(r"#define\s+SOW_DTYPE_F16\s+(\d+)", header)
    assert m is not None and int(m.group(1)) == _lib.F16 == 2
    assert _lib.load().sow_version() >= 112


def test_f16_workspace_queries_are_nonzero():
    lib = __import__("sow_amd._lib", fromlist=["load"]).load()
    assert lib.sow_workspace_bytes(32768, 512, 512, 50, 0, 0, 2) > 0
    assert lib.sow_workspace_bytes(32768, 512, 512, 50, 0, 2, 2) > 0
    # an unknown dtype is still refused
    assert lib.sow_workspace_bytes(32768, 512, 512, 50, 0, 0, 3) == 0


def test_f16_forward_checks_pointers_not_dtype():
    from sow_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    rc = lib.sow_forward(null, null, null, null, null, null, null, null, 64, 512, 512, 8, 0, 0, 1.0, _lib.F16, null, 0,
                         null)
    assert rc == -1, lib.sow_error_string(rc)   # SOW_ERR_NULL, not SOW_ERR_DTYPE (-3)
    rc = lib.sow_forward(null, null, null, null, null, null, null, null, 64, 512, 512, 8, 0, 0, 1.0, 3, null, 0, null)
    assert rc == -3
    rc = lib.sow_backward(null, null, null, null, null, null, null, null, null, null, null, 64, 512, 512, 8, 0, 0, 1.0,
                          0.0, _lib.F16, null, 0, null)
    assert rc == -1


def test_ops_maps_float16_tensors():
    from sow_amd import _lib, ops
    assert ops._dt(torch.empty(2, dtype=torch.float16)) == _lib.F16
    assert ops._dt(torch.empty(2, dtype=torch.bfloat16)) == _lib.BF16
    try:
        ops._dt(torch.empty(2, dtype=torch.float64))
    except TypeError as e:
        assert "float16" in str(e)
    else:
        raise AssertionError("float64 must be refused")
