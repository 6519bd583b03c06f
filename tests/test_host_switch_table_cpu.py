"""CPU tests of the kernel-selection switch table: kSwitchNames (api.hip) and enum Switch (common.hpp) stay parallel, the cache
and store switches of the chain and weight-gradient kernels (NO_H_ROWS, NT_LOAD, TN_NO_NT_LOAD, NO_NT_STORE) and the launch-shape
and dispatch switches the GPU tests set (NO_PERSIST, NO_PAIR_FLUSH, NO_PARK16, NO_SHORT_SPLIT, FORCE_GEMM_V1, NO_GEMM3S) exist, are
unset unless the environment sets them and can be set and restored, each on its own, and the C ABI carries no policy parameter (header and _lib.py
stay one to one)."""
import ctypes
import os
import re

from sow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the cache / store policies, then the launch-shape and dispatch switches the GPU tests set (test_gpu_stream_policy.py,
# test_gpu_elementwise.py)
SWITCHES = ("NO_H_ROWS", "NT_LOAD", "TN_NO_NT_LOAD", "NO_NT_STORE", "NO_PERSIST", "NO_PAIR_FLUSH", "NO_PARK16", "NO_SHORT_SPLIT",
            "FORCE_GEMM_V1", "NO_GEMM3S")


def test_switches_exist_and_default_to_unset():
    lib = _lib.load()
    for name in SWITCHES:
        assert lib.sow_get_switch(name.encode()) in (-1, 0, 1), name
        if ("SOW_AMD_" + name) not in os.environ:
            assert lib.sow_get_switch(name.encode()) == -1, name
    assert lib.sow_get_switch(b"NO_SUCH_POLICY") == -6


def test_switches_set_and_restore():
    lib = _lib.load()
    before = {n: lib.sow_get_switch(n.encode()) for n in SWITCHES}
    with _lib.switch(NO_H_ROWS=1, NT_LOAD=1):
        assert lib.sow_get_switch(b"NO_H_ROWS") == 1 and lib.sow_get_switch(b"NT_LOAD") == 1
        with _lib.switch(NO_H_ROWS=0):
            assert lib.sow_get_switch(b"NO_H_ROWS") == 0 and lib.sow_get_switch(b"NT_LOAD") == 1
        assert lib.sow_get_switch(b"NO_H_ROWS") == 1
    assert {n: lib.sow_get_switch(n.encode()) for n in SWITCHES} == before
    for n in SWITCHES:                       # every name round-trips on its own: set, read back, cleared, restored
        for v in (1, 0):
            with _lib.switch(**{n: v}):
                assert lib.sow_get_switch(n.encode()) == v, n
                assert all(lib.sow_get_switch(o.encode()) == before[o] for o in SWITCHES if o != n), n
        assert lib.sow_get_switch(n.encode()) == before[n], n


def test_switch_names_match_the_enum():
    """kSwitchNames (api.hip) and enum Switch (common.hpp) are parallel lists: same length, same order."""
    csrc = os.path.join(ROOT, "sow_amd", "csrc")
    enum = re.search(r"enum Switch : int \{(.*?)SW_COUNT", open(os.path.join(csrc, "common.hpp")).read(), re.S).group(1)
    enum_names = re.findall(r"^\s*SW_([A-Z0-9_]+)\s*(?:=\s*0\s*)?,", re.sub(r"//.*", "", enum), re.M)
    table = re.search(r"kSwitchNames\[SW_COUNT\] = \{(.*?)\};", open(os.path.join(csrc, "api.hip")).read(), re.S).group(1)
    assert re.findall(r'"([A-Z0-9_]+)"', table) == enum_names
    assert enum_names[-1] == "NO_H_ROWS"


def test_c_abi_is_unchanged_and_one_to_one():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sow_amd.h")).read(), flags=re.S)
    header = re.sub(r"//.*", "", header)
    declared = set(re.findall(r"\b(sow_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert not any("policy" in n or "stream_sw" in n for n in declared)   # the policy is not a caller-visible parameter
