"""CPU table test of the host dispatch of the C ABI (sow_amd/csrc/api.hip; no GPU compute): the full plan surface
(workspace queries, reduce descriptors, group plans) and the return code, with its precedence when a call has two defects,
of every layer entry point -- for calls that return before any launch.  The expected values are a recording of the library
(tests/golden/host_dispatch_table.json), made with fake pointers so that descriptor bytes are reproducible:

    python tests/test_host_dispatch_table_cpu.py --record

The recorder refuses a row whose code is positive (a HIP error: a launch was attempted); such a row is taken out of the
generator, never skipped at test time."""
import ctypes
import hashlib
import itertools
import json
import os
import re
import sys
import zlib
import base64

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from sow_amd import _lib  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "host_dispatch_table.json")
FAKE = 0x10000          # never dereferenced: every recorded call returns before a launch
BIG = 1 << 40           # a workspace size no plan exceeds
F32, BF16, F16, PF, FUSE = _lib.F32, _lib.BF16, _lib.F16, _lib.PARAM_F32, _lib.FUSE_ACC
NONE, LOWRANK, DENSE = _lib.ACC_NONE, _lib.ACC_LOWRANK, _lib.ACC_DENSE
DATA, WEIGHTS, PARTIAL, REDUCE, SLABS = (_lib.BWD_DATA, _lib.BWD_WEIGHTS, _lib.BWD_WEIGHTS_PARTIAL, _lib.BWD_WEIGHTS_REDUCE,
                                         _lib.BWD_GROUP_SLABS)
DTYPE_NAMES = {F32: "f32", BF16: "bf16", F16: "f16", BF16 | PF: "bf16+pf", F16 | PF: "f16+pf", BF16 | FUSE: "bf16+fuse",
               F32 | PF: "f32+pf", 99: "d99", 99 | PF: "d99+pf"}

# ---- workspace queries ------------------------------------------------------------------------------------------------
WS_T = (0, 1, 64, 1000, 8192, 8193, 32768)
WS_SHAPES = ((512, 512), (512, 1376), (1376, 512), (2048, 5461), (100, 36), (4096, 4096))
WS_R = (8, 50, 63, 64, 66, 200, 256)
WS_ACC = ((NONE, 0), (DENSE, 0), (LOWRANK, 32), (LOWRANK, 100), (LOWRANK, 200))
WS_DTYPES = (F32, BF16, F16, BF16 | PF, F16 | PF, BF16 | FUSE, F32 | PF, 99)


def _ws_grid():
    return itertools.product(WS_T, WS_SHAPES, WS_R, WS_ACC, WS_DTYPES)


def _workspace_rows(lib):
    """The two layer queries over the whole grid, as flat lists in _ws_grid() order, and a small grid of the others."""
    out = {"sow_workspace_bytes": [], "sow_forward_workspace_bytes": []}
    for T, (d_in, d_out), r, (kind, r_acc), dt in _ws_grid():
        for name in out:
            out[name].append(getattr(lib, name)(T, d_in, d_out, r, r_acc, kind, dt))
    small = {}
    for T, (d_in, d_out), r, kind, dt in itertools.product((0, 1, 8, 32, 33), ((512, 512), (2048, 5464), (100, 36)), (8, 64, 66),
                                                           (NONE, DENSE, LOWRANK), (F32, BF16, F16, BF16 | PF, BF16 | FUSE)):
        small[f"skinny T={T} {d_in}x{d_out} r={r} acc={kind} {DTYPE_NAMES[dt]}"] = \
            lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt)
    for M, (N, K), ta, dt in itertools.product((0, 64, 1024, 32768), ((512, 512), (5461, 2048), (4096, 4096)), (0, 1),
                                               (F32, BF16, F16, BF16 | FUSE)):
        small[f"gemm M={M} N={N} K={K} ta={ta} {DTYPE_NAMES[dt]}"] = lib.sow_gemm_workspace_bytes(M, N, K, ta, dt)
    for (m, n, k), dt, need_r in itertools.product(((512, 64, 50), (2048, 5461, 256), (2048, 200, 200), (100, 36, 36), (0, 4, 4)),
                                                   (F32, BF16, F16, BF16 | FUSE), (0, 1)):
        small[f"qr m={m} n={n} k={k} {DTYPE_NAMES[dt]} need_r={need_r}"] = lib.sow_qr_workspace_bytes(m, n, k, dt, need_r)
    for T, r in itertools.product((0, 1, 1000, 32768), (8, 63, 64, 66, 256)):
        small[f"h_save T={T} r={r}"] = lib.sow_h_save_elems(T, r)
    out["small"] = small
    return out


# ---- layers -------------------------------------------------------------------------------------------------------------
PTRS = ("x", "A", "B", "y", "h_save", "dy", "dx", "dA", "dB", "workspace")


def _layer(**over):
    """A complete, valid 1024 x 512 x 512 layer of rank 50 on fake pointers (no accumulator, no bias), then `over`."""
    L = _lib.LayerArgs()
    for f in PTRS:
        setattr(L, f, FAKE)
    L.T, L.d_in, L.d_out, L.r_live, L.r_acc, L.acc_kind = 1024, 512, 512, 50, 0, NONE
    L.scale, L.grad_beta, L.workspace_bytes = 0.5, 1.0, BIG
    for k, v in over.items():
        setattr(L, k, v)
    return L


def _arr(layers):
    arr = (_lib.LayerArgs * max(len(layers), 1))()
    for i, L in enumerate(layers):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(L), ctypes.sizeof(L))
    return arr


def _forward(lib, L, dt):
    return lib.sow_forward(L.x, L.A, L.B, L.acc_down, L.acc_up, L.bias, L.y, L.h_save, L.T, L.d_in, L.d_out, L.r_live, L.r_acc,
                           L.acc_kind, L.scale, dt, L.workspace, L.workspace_bytes, None)


def _backward(lib, L, dt, phases):
    return lib.sow_backward_ex(L.dy, L.x, L.h_save, L.A, L.B, L.acc_down, L.acc_up, L.dx, L.dA, L.dB, L.dbias, L.T, L.d_in,
                               L.d_out, L.r_live, L.r_acc, L.acc_kind, L.scale, L.grad_beta, dt, L.workspace, L.workspace_bytes,
                               phases, None)


def _need(lib, L, dt, phases):
    """The smallest workspace_bytes the backward of L accepts (sow_workspace_bytes counts one byte of slack more): the
    plan of the compute dtype -- SOW_FUSE_ACC is a permission, a call without it must fit -- and, in the phase that packs
    the fp32 parameters, the packed copies."""
    dt &= ~FUSE
    if not phases & DATA:
        dt &= ~PF
    return lib.sow_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, L.r_acc, L.acc_kind, dt) - 1


# one defect each; the value is the keyword set applied to _layer()
SHAPE_DEFECTS = {"T=-1": dict(T=-1), "d_in=0": dict(d_in=0), "d_in=-1": dict(d_in=-1), "d_out=0": dict(d_out=0),
                 "d_out=-3": dict(d_out=-3), "r_live=0": dict(r_live=0), "r_live=-1": dict(r_live=-1)}
ACC_DEFECTS = {"dense acc_down=NULL": dict(acc_kind=DENSE), "lowrank acc_down=NULL": dict(acc_kind=LOWRANK, acc_up=FAKE, r_acc=32),
               "lowrank acc_up=NULL": dict(acc_kind=LOWRANK, acc_down=FAKE, r_acc=32),
               "lowrank r_acc=0": dict(acc_kind=LOWRANK, acc_down=FAKE, acc_up=FAKE, r_acc=0),
               "lowrank r_acc=-1": dict(acc_kind=LOWRANK, acc_down=FAKE, acc_up=FAKE, r_acc=-1),
               "lowrank acc_up=NULL acc_down=NULL": dict(acc_kind=LOWRANK, r_acc=32)}
# what only the per-layer fall-through of a group tests (check_layer does not look at a low-rank accumulator's second factor)
FALL_THROUGH_ONLY = ("lowrank acc_up=NULL", "lowrank r_acc=0", "lowrank r_acc=-1")
FWD_PTRS = ("x", "A", "B", "y")
BWD_PTRS = ("dy", "x", "h_save", "A", "B", "dx", "dA", "dB", "workspace")
LAYER_DTYPES = (BF16, BF16 | PF, F16, F16 | PF, F32, BF16 | FUSE)        # unflagged and flagged
BAD_DTYPES = (99, 99 | PF, F32 | PF)
PHASE_SETS = {"data+weights": DATA | WEIGHTS, "data": DATA, "weights": WEIGHTS, "partial": PARTIAL, "reduce": REDUCE,
              "data+partial": DATA | PARTIAL}


def _layer_defects(bwd):
    """name -> keyword set: one defect each, then the pairs that pin which defect wins."""
    d = {}
    for p in (BWD_PTRS if bwd else FWD_PTRS):
        d[f"{p}=NULL"] = {p: None}
    d.update(SHAPE_DEFECTS)
    d.update(ACC_DEFECTS)
    d["d_in=0 x=NULL"] = dict(d_in=0, x=None)                       # bad shape with NULL
    d["r_live=0 A=NULL B=NULL"] = dict(r_live=0, A=None, B=None)
    d["T=-1 lowrank acc_up=NULL"] = dict(T=-1, acc_kind=LOWRANK, acc_down=FAKE, r_acc=32)
    d["x=NULL lowrank r_acc=0"] = dict(x=None, acc_kind=LOWRANK, acc_down=FAKE, acc_up=FAKE, r_acc=0)
    d["dense acc_down=NULL d_out=0"] = dict(acc_kind=DENSE, d_out=0)
    # T = 0 launches nothing (backward: grad_beta = 1 leaves the gradients as they are), whatever else is NULL
    d["T=0"] = dict(T=0)
    d["T=0 x=NULL y=NULL dy=NULL dx=NULL workspace=NULL"] = dict(T=0, x=None, y=None, dy=None, dx=None, workspace=None)
    d["T=0 d_in=0"] = dict(T=0, d_in=0)
    d["T=0 lowrank acc_up=NULL"] = dict(T=0, acc_kind=LOWRANK, acc_down=FAKE, r_acc=32)
    if bwd:
        d["T=0 dA=NULL"] = dict(T=0, dA=None)
        d["T=0 dB=NULL"] = dict(T=0, dB=None)
    return d


def _single_rows(lib):
    rows = {}
    for dt in LAYER_DTYPES:
        dn = DTYPE_NAMES[dt]
        for name, over in _layer_defects(False).items():
            rows[f"sow_forward {dn} {name}"] = _forward(lib, _layer(**over), dt)
        if dt & PF:
            # the packed parameters need a workspace; the unflagged forward of this shape needs none
            rows[f"sow_forward {dn} workspace=NULL"] = _forward(lib, _layer(workspace=None), dt)
            fq = lib.sow_forward_workspace_bytes(1024, 512, 512, 50, 0, NONE, dt)
            rows[f"sow_forward {dn} workspace one byte short"] = _forward(lib, _layer(workspace_bytes=fq - 2), dt)
            rows[f"sow_forward {dn} workspace_bytes=0"] = _forward(lib, _layer(workspace_bytes=0), dt)
        if dt in (BF16, F16):
            # a wide low-rank accumulator and a wide live term without h_save compose through the workspace
            wide_acc = dict(acc_kind=LOWRANK, acc_down=FAKE, acc_up=FAKE, r_acc=100)
            rows[f"sow_forward {dn} r_acc=100 workspace=NULL"] = _forward(lib, _layer(workspace=None, **wide_acc), dt)
            rows[f"sow_forward {dn} r_acc=100 workspace_bytes=0"] = _forward(lib, _layer(workspace_bytes=0, **wide_acc), dt)
            rows[f"sow_forward {dn} r_live=200 h_save=NULL workspace=NULL"] = \
                _forward(lib, _layer(r_live=200, h_save=None, workspace=None), dt)
            rows[f"sow_forward {dn} r_live=200 h_save=NULL workspace_bytes=0"] = \
                _forward(lib, _layer(r_live=200, h_save=None, workspace_bytes=0), dt)
        for pn, ph in PHASE_SETS.items():
            for name, over in _layer_defects(True).items():
                rows[f"sow_backward_ex {dn} {pn} {name}"] = _backward(lib, _layer(**over), dt, ph)
            for kind, extra in ((NONE, {}), (DENSE, dict(acc_down=FAKE)), (LOWRANK, dict(acc_down=FAKE, acc_up=FAKE, r_acc=100))):
                L = _layer(acc_kind=kind, **extra)
                L.workspace_bytes = _need(lib, L, dt, ph) - 1
                rows[f"sow_backward_ex {dn} {pn} acc={kind} workspace one byte short"] = _backward(lib, L, dt, ph)
            rows[f"sow_backward_ex {dn} {pn} workspace_bytes=0"] = _backward(lib, _layer(workspace_bytes=0), dt, ph)
        for ph in (0, SLABS):
            rows[f"sow_backward_ex {dn} phases={ph}"] = _backward(lib, _layer(), dt, ph)
            rows[f"sow_backward_ex {dn} phases={ph} d_in=0"] = _backward(lib, _layer(d_in=0), dt, ph)
            rows[f"sow_backward_ex {dn} phases={ph} x=NULL"] = _backward(lib, _layer(x=None), dt, ph)
            rows[f"sow_backward_ex {dn} phases={ph} T=0"] = _backward(lib, _layer(T=0), dt, ph)
    for dt in BAD_DTYPES:
        dn = DTYPE_NAMES[dt]
        for name, over in (("", {}), (" d_in=0", dict(d_in=0)), (" x=NULL", dict(x=None)), (" T=0", dict(T=0)), (" T=-1", dict(T=-1)),
                           (" lowrank r_acc=0", dict(acc_kind=LOWRANK, acc_down=FAKE, acc_up=FAKE, r_acc=0))):
            rows[f"sow_forward {dn}{name}"] = _forward(lib, _layer(**over), dt)
            for ph in (DATA | WEIGHTS, PARTIAL, 0):
                rows[f"sow_backward_ex {dn} phases={ph}{name}"] = _backward(lib, _layer(**over), dt, ph)
    return rows


def _group_rows(lib):
    rows = {}
    entry = {"sow_forward_group": (False, lambda a, n, dt, ph: lib.sow_forward_group(a, n, dt, None)),
             "sow_backward_group": (True, lambda a, n, dt, ph: lib.sow_backward_group(a, n, dt, ph, None)),
             "sow_forward_shared": (False, lambda a, n, dt, ph: lib.sow_forward_shared(a, n, dt, None)),
             "sow_backward_shared": (True, lambda a, n, dt, ph: lib.sow_backward_shared(a, n, dt, ph, None))}
    for fn, (bwd, call) in entry.items():
        shared = "shared" in fn
        phase_sets = PHASE_SETS if bwd else {"-": 0}
        for dt in LAYER_DTYPES + BAD_DTYPES:
            dn = DTYPE_NAMES[dt]
            for pn, ph in phase_sets.items():
                key = f"{fn} {dn} {pn}"
                rows[f"{key} n=-1"] = call(_arr([_layer()]), -1, dt, ph)
                rows[f"{key} n=0"] = call(_arr([_layer()]), 0, dt, ph)
                rows[f"{key} layers=NULL"] = call(None, 2, dt, ph)
                rows[f"{key} layers=NULL n=-1"] = call(None, -1, dt, ph)
                empty = _layer(T=0)
                for name, over in _layer_defects(bwd).items():
                    if shared and "T" in over:
                        continue          # siblings share T: the sets below
                    if bwd and name in FALL_THROUGH_ONLY and ph & (WEIGHTS | PARTIAL) and not ph & DATA:
                        continue          # the grouped weight-gradient launch reads no accumulator: it takes the layer
                    bad = _layer(**over)
                    rows[f"{key} layer0: {name}"] = call(_arr([bad, empty if not shared else _layer()]), 2, dt, ph)
                    if not shared:
                        # the defective layer behind layers that launch nothing
                        rows[f"{key} layer2 of T=0,T=0: {name}"] = call(_arr([empty, empty, bad]), 3, dt, ph)
                if not shared:
                    rows[f"{key} all T=0"] = call(_arr([empty, empty]), 2, dt, ph)
                if bwd and not shared:
                    if dt in LAYER_DTYPES:
                        L = _layer()
                        L.workspace_bytes = _need(lib, L, dt, ph) - 1
                        rows[f"{key} layer0: workspace one byte short"] = call(_arr([L, empty]), 2, dt, ph)
                    rows[f"{key} layer0: workspace_bytes=0"] = call(_arr([_layer(workspace_bytes=0)]), 1, dt, ph)
            if bwd:
                for ph in (0, SLABS):
                    rows[f"{fn} {dn} phases={ph}"] = call(_arr([_layer(), _layer()]), 2, dt, ph)
                    rows[f"{fn} {dn} phases={ph} n=-1"] = call(_arr([_layer()]), -1, dt, ph)
                    rows[f"{fn} {dn} phases={ph} layers=NULL"] = call(None, 2, dt, ph)
                    rows[f"{fn} {dn} phases={ph} layer0: d_in=0"] = call(_arr([_layer(d_in=0), _layer()]), 2, dt, ph)
            if not shared:
                continue
            ph = DATA | WEIGHTS
            key = f"{fn} {dn}"
            rows[f"{key} n=5"] = call(_arr([_layer()] * 5), 5, dt, ph)
            rows[f"{key} n=5 layer4: x=NULL"] = call(_arr([_layer()] * 4 + [_layer(x=None)]), 5, dt, ph)
            rows[f"{key} n=5 layer4: A=NULL"] = call(_arr([_layer()] * 4 + [_layer(A=None)]), 5, dt, ph)
            rows[f"{key} other x"] = call(_arr([_layer(), _layer(x=FAKE + 4096)]), 2, dt, ph)
            rows[f"{key} other T"] = call(_arr([_layer(), _layer(T=2048)]), 2, dt, ph)
            rows[f"{key} other d_in"] = call(_arr([_layer(), _layer(d_in=1376)]), 2, dt, ph)
            rows[f"{key} other d_in, layer1: A=NULL"] = call(_arr([_layer(), _layer(d_in=1376, A=None)]), 2, dt, ph)
            rows[f"{key} other dx"] = call(_arr([_layer(), _layer(dx=FAKE + 4096)]), 2, dt, ph)
            rows[f"{key} layer1: dx=NULL"] = call(_arr([_layer(), _layer(dx=None)]), 2, dt, ph)
            rows[f"{key} all T=0"] = call(_arr([_layer(T=0), _layer(T=0)]), 2, dt, ph)
            rows[f"{key} all T=-1"] = call(_arr([_layer(T=-1), _layer(T=-1)]), 2, dt, ph)
            rows[f"{key} all T=0, layer1: d_out=0"] = call(_arr([_layer(T=0), _layer(T=0, d_out=0)]), 2, dt, ph)
            rows[f"{key} T=1024 is not admitted"] = call(_arr([_layer(), _layer()]), 2, dt, ph)
            rows[f"{key} dense accumulator is not admitted"] = \
                call(_arr([_layer(T=16384, acc_kind=DENSE, acc_down=FAKE)] * 2), 2, dt, ph)
            rows[f"{key} r_live=200 is not admitted"] = call(_arr([_layer(T=16384, r_live=200)] * 2), 2, dt, ph)
            rows[f"{key} misaligned B is not admitted"] = call(_arr([_layer(T=16384), _layer(T=16384, B=FAKE + 8)]), 2, dt, ph)
            if bwd:
                rows[f"{key} layer1: workspace_bytes=0"] = \
                    call(_arr([_layer(T=16384), _layer(T=16384, workspace_bytes=0)]), 2, dt, ph)
    return rows


def _skinny_rows(lib):
    rows = {}

    def sk(**over):
        L = _layer(**dict(dict(T=8), **over))
        if "workspace_bytes" not in over:
            L.workspace_bytes = lib.sow_forward_skinny_workspace_bytes(L.T, L.d_in, L.d_out, L.r_live, L.acc_kind, BF16)
        return L

    def call(layers, n, dt):
        return lib.sow_forward_skinny(None if layers is None else _arr(layers), n, dt, None)

    for dt in (BF16, F16, BF16 | FUSE, BF16 | PF, F16 | PF, F32, F32 | PF, 99, 99 | PF):
        key = f"sow_forward_skinny {DTYPE_NAMES[dt]}"
        rows[f"{key} n=-1"] = call([sk()], -1, dt)
        rows[f"{key} n=0"] = call([sk()], 0, dt)
        rows[f"{key} layers=NULL"] = call(None, 2, dt)
        rows[f"{key} n=17"] = call([sk()] * 17, 17, dt)
        rows[f"{key} n=17 layer0: d_in=0"] = call([sk(d_in=0)] * 17, 17, dt)
        defects = dict(SHAPE_DEFECTS)
        for p in FWD_PTRS:
            defects[f"{p}=NULL"] = {p: None}
        for p in ("x", "y", "A", "B"):
            defects[f"{p} misaligned"] = {p: FAKE + 8}
        defects.update({
            "bias misaligned": dict(bias=FAKE + 2), "dense acc_down=NULL": dict(acc_kind=DENSE),
            "dense acc_down misaligned": dict(acc_kind=DENSE, acc_down=FAKE + 4), "acc_kind=7": dict(acc_kind=7),
            "acc_kind=7 T=0": dict(acc_kind=7, T=0), "lowrank": dict(acc_kind=LOWRANK, acc_down=FAKE, acc_up=FAKE, r_acc=32),
            "T=33": dict(T=33), "r_live=66": dict(r_live=66), "d_in=100": dict(d_in=100), "d_out=36": dict(d_out=36),
            "workspace=NULL": dict(workspace=None), "workspace_bytes=0": dict(workspace_bytes=0),
            "T=33 x=NULL": dict(T=33, x=None), "x=NULL x misaligned elsewhere": dict(x=None, y=FAKE + 8),
            "y misaligned workspace=NULL": dict(y=FAKE + 8, workspace=None), "d_in=0 acc_kind=7": dict(d_in=0, acc_kind=7),
            "T=0 d_in=0": dict(T=0, d_in=0)})
        for name, over in defects.items():
            rows[f"{key} layer0: {name}"] = call([sk(**over), sk()], 2, dt)
            rows[f"{key} layer1: {name}"] = call([sk(), sk(**over)], 2, dt)
        for kind, extra in ((NONE, {}), (DENSE, dict(acc_down=FAKE))):
            L = sk(acc_kind=kind, **extra)
            L.workspace_bytes -= 1
            rows[f"{key} acc={kind} workspace one byte short"] = call([sk(), L], 2, dt)
    return rows


# ---- reduce descriptors and group plans ---------------------------------------------------------------------------------
def _sha(raw):
    return hashlib.sha256(raw).hexdigest()


def _reduce_desc_rows(lib):
    rows = {}
    size = lib.sow_reduce_desc_bytes()
    for r, dbias, dt, (T, d_in, d_out), short in itertools.product((50, 63, 64, 200), (None, FAKE + 0x400), (BF16, F32, BF16 | PF),
                                                                   ((1024, 512, 512), (32768, 512, 1376)), (False, True)):
        need = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, NONE, dt & ~PF) - 1
        desc = ctypes.create_string_buffer(b"\xaa" * size, size)
        blocks = ctypes.c_int(-7)
        rc = lib.sow_backward_reduce_desc(FAKE, FAKE + 0x100, dbias, T, d_in, d_out, r, 0, NONE, 1.0, dt, FAKE + 0x1000,
                                          need - 1 if short else need, desc, ctypes.byref(blocks))
        rows[f"r={r} dbias={'yes' if dbias else 'no'} {DTYPE_NAMES[dt]} {T}x{d_in}x{d_out}{' one byte short' if short else ''}"] = \
            [rc, blocks.value, _sha(desc.raw)]
    for name, kw in {"dtype 99": dict(dt=99), "T=0": dict(T=0), "dA=NULL": dict(dA=None), "desc=NULL": dict(desc=False),
                     "d_in=0 dA=NULL": dict(d_in=0, dA=None), "dtype 99 T=0": dict(dt=99, T=0)}.items():
        a = dict(dA=FAKE, T=1024, d_in=512, dt=BF16, desc=True)
        a.update(kw)
        desc = ctypes.create_string_buffer(size)
        blocks = ctypes.c_int(-7)
        rows[name] = [lib.sow_backward_reduce_desc(a["dA"], FAKE, None, a["T"], a["d_in"], 512, 50, 0, NONE, 1.0, a["dt"], FAKE, BIG,
                                                   desc if a["desc"] else None, ctypes.byref(blocks)), blocks.value]
    return rows


BLOCKS = {"llama_60m": (512, 1376), "llama_1b": (2048, 5461)}


def _block(lib, hidden, inter, T, r, dt):
    """The seven SoW layers of a llama decoder block (q, k, v, o; gate, up; down), each with its own fake buffers."""
    shapes = [(hidden, hidden)] * 4 + [(hidden, inter), (hidden, inter), (inter, hidden)]
    layers = []
    for i, (d_in, d_out) in enumerate(shapes):
        L = _layer(T=T, d_in=d_in, d_out=d_out, r_live=r)
        for j, f in enumerate(PTRS):
            setattr(L, f, FAKE * (16 * i + j + 1))
        L.workspace_bytes = lib.sow_workspace_bytes(T, d_in, d_out, r, 0, NONE, dt)
        layers.append(L)
    return _arr(layers), len(shapes)


def _group_plan_rows(lib):
    rows = {}
    size = lib.sow_reduce_desc_bytes()
    for (model, (hidden, inter)), T, r, dt, ph in itertools.product(
            BLOCKS.items(), (1024, 32768), (50, 200), (BF16, F16, F32, BF16 | PF),
            (DATA | WEIGHTS, PARTIAL, PARTIAL | SLABS, REDUCE | SLABS)):
        arr, n = _block(lib, hidden, inter, T, r, dt)
        slabs = (ctypes.c_int * (2 * n))(*([-7] * (2 * n)))
        rc_plan = lib.sow_backward_group_plan(arr, n, dt, ph, slabs)
        descs = ctypes.create_string_buffer(b"\xaa" * (n * size), n * size)
        blocks = (ctypes.c_int * n)(*([-7] * n))
        rc_desc = lib.sow_backward_group_reduce_desc(arr, n, dt, ph, descs, blocks)
        rows[f"{model} T={T} r={r} {DTYPE_NAMES[dt]} phases={ph}"] = [rc_plan, list(slabs), rc_desc, list(blocks), _sha(descs.raw)]
    arr, n = _block(lib, 512, 1376, 1024, 50, BF16)
    for name, (a, m, dt) in {"n=-1": (arr, -1, BF16), "n=0": (arr, 0, BF16), "layers=NULL": (None, n, BF16), "dtype 99": (arr, n, 99),
                             "dtype 99 n=-1": (arr, -1, 99), "layer0: dA=NULL": (_arr([_layer(dA=None)]), 1, BF16),
                             "layer0: d_in=0 dA=NULL": (_arr([_layer(d_in=0, dA=None)]), 1, BF16),
                             "n=9": (_arr([_layer()] * 9), 9, BF16)}.items():
        descs = ctypes.create_string_buffer(9 * size)
        blocks = (ctypes.c_int * 9)()
        rows[name] = [lib.sow_backward_group_plan(a, m, dt, PARTIAL | SLABS, None),
                      lib.sow_backward_group_reduce_desc(a, m, dt, PARTIAL | SLABS, descs, blocks)]
    return rows


# ---- the table ----------------------------------------------------------------------------------------------------------
def _switch_names():
    table = re.search(r"kSwitchNames\[SW_COUNT\] = \{(.*?)\};", open(os.path.join(ROOT, "sow_amd", "csrc", "api.hip")).read(), re.S)
    return re.findall(r'"([A-Z0-9_]+)"', table.group(1))


def _set_switches(lib):
    return [n for n in _switch_names() if lib.sow_get_switch(n.encode()) != -1]


SECTIONS = {"workspace": _workspace_rows, "reduce_desc": _reduce_desc_rows, "group_plan": _group_plan_rows,
            "codes_single": _single_rows, "codes_group": _group_rows, "codes_skinny": _skinny_rows}


def _codes_of(section, rows):
    """Every return code of a section, for the recorder's positive-code refusal."""
    if section.startswith("codes_"):
        return {k: [v] for k, v in rows.items()}
    if section == "reduce_desc":
        return {k: [v[0]] for k, v in rows.items()}
    if section == "group_plan":
        # sow_backward_group_plan returns 1 for "the row-owner kernel runs": not a code
        return {k: [min(v[0], 0), v[2] if len(v) == 5 else v[1]] for k, v in rows.items()}
    return {}


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    names = _switch_names()
    assert len(names) > 20
    on = _set_switches(lib)
    if on:
        env = [n for n in on if ("SOW_AMD_" + n) in os.environ]
        if env:
            pytest.skip(f"the table is recorded under default switches; the environment sets SOW_AMD_{env[0]}")
        assert not on, f"a switch was left set: {on}"
    return lib


# ---- the fixture's form ---------------------------------------------------------------------------------------------------
# The generator names every row; the fixture holds the values alone, in the generator's order, with a SHA-256 of the names so
# that a generator and a fixture that list different rows cannot be compared.  Return codes (0 .. -6) are one digit each; the
# two workspace grids (11760 sizes each) are the zlib-compressed JSON list in base64.  Long strings are cut into lines.
def _lines(s, n=120):
    return [s[i:i + n] for i in range(0, len(s), n)]


def _keyed(rows, codes=False):
    vals = list(rows.values())
    if codes:
        assert all(-6 <= v <= 0 for v in vals)
        vals = _lines("".join(str(-v) for v in vals))
    return {"names_sha256": _sha("\n".join(rows).encode()), "values": vals}


def _unkeyed(stored, names, codes=False):
    assert stored["names_sha256"] == _sha("\n".join(names).encode()), "the generator and the fixture list different rows: record again"
    vals = [-int(c) for c in "".join(stored["values"])] if codes else stored["values"]
    assert len(vals) == len(names)
    return dict(zip(names, vals))


def _pack(table):
    out = {}
    for section, rows in table.items():
        if section == "workspace":
            out[section] = {k: _lines(base64.b64encode(zlib.compress(json.dumps(v, separators=(",", ":")).encode(), 9)).decode())
                            for k, v in rows.items() if k != "small"}
            out[section]["small"] = _keyed(rows["small"])
        else:
            out[section] = _keyed(rows, section.startswith("codes_"))
    return out


def _dump(packed, depth=0):
    """JSON with one line per row or string piece (lists inside a row stay on its line)."""
    if isinstance(packed, dict):
        return "{\n" + ",\n".join(f"{json.dumps(k)}: {_dump(v, depth + 1)}" for k, v in packed.items()) + "\n}"
    if isinstance(packed, list) and len(packed) > 16:
        rows = [json.dumps(packed[i:i + 16], separators=(",", ":"))[1:-1] if isinstance(packed[0], int) else
                json.dumps(packed[i], separators=(",", ":")) for i in range(0, len(packed), 16 if isinstance(packed[0], int) else 1)]
        return "[\n" + ",\n".join(rows) + "\n]"
    return json.dumps(packed, separators=(",", ":"))


def _unpack(stored, got):
    """The fixture as the generators return a table; `got` (this build's table) supplies the row names."""
    out = {}
    for section, rows in stored.items():
        if section == "workspace":
            out[section] = {k: json.loads(zlib.decompress(base64.b64decode("".join(v)))) for k, v in rows.items() if k != "small"}
            out[section]["small"] = _unkeyed(rows["small"], list(got[section]["small"]))
        else:
            out[section] = _unkeyed(rows, list(got[section]), section.startswith("codes_"))
    return out


@pytest.fixture(scope="module")
def tables(lib):
    got = {s: json.loads(json.dumps(make(lib))) for s, make in SECTIONS.items()}      # tuples / ints as JSON has them
    with open(FIXTURE) as f:
        return got, _unpack(json.load(f), got)


@pytest.fixture(scope="module")
def golden(tables):
    return tables[1]


@pytest.mark.parametrize("section", list(SECTIONS))
def test_dispatch_table(tables, section):
    got, want = tables[0][section], tables[1][section]
    assert sorted(got) == sorted(want), "the generator and the fixture list different rows: record again"
    if section == "workspace":
        grid = list(_ws_grid())
        for name in ("sow_workspace_bytes", "sow_forward_workspace_bytes"):
            assert len(got[name]) == len(want[name]) == len(grid)
            bad = [(grid[i], got[name][i], want[name][i]) for i in range(len(grid)) if got[name][i] != want[name][i]]
            assert not bad, f"{name}: {len(bad)} rows differ, first (T, shape, r, acc, dtype), got, want = {bad[0]}"
        got, want = got["small"], want["small"]
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"{len(bad)} of {len(want)} rows differ, first (got, want): {next(iter(bad.items()))}"
    for k, codes in _codes_of(section, got).items():
        assert all(c <= 0 for c in codes), f"{k}: a launch was attempted"


def test_table_has_the_rows_the_refactor_depends_on(golden):
    """The fixture is the whole grid, and holds every class of row (nothing dropped at recording time)."""
    assert len(golden["workspace"]["sow_workspace_bytes"]) == len(list(_ws_grid())) == 7 * 6 * 7 * 5 * 8
    singles, groups = golden["codes_single"], golden["codes_group"]
    assert singles["sow_backward_ex bf16 phases=0 d_in=0"] == _lib.ERR_SHAPE
    for fn in ("sow_forward", "sow_forward_group", "sow_backward_group", "sow_forward_shared", "sow_backward_shared",
               "sow_backward_ex", "sow_forward_skinny"):
        for dn in ("bf16", "bf16+pf"):
            both = dict(singles, **groups, **golden["codes_skinny"])
            assert any(k.startswith(f"{fn} {dn} ") for k in both), (fn, dn)
    assert any(v == 0 for k, v in singles.items() if " T=0" in k)
    assert any(v[0] == 1 for v in golden["group_plan"].values() if len(v) == 5)


def record():
    lib = _lib.load()
    on = _set_switches(lib)
    if on:
        raise SystemExit(f"record under default switches only; set: {on}")
    table = {}
    for section, make in SECTIONS.items():
        rows = make(lib)
        refused = {k: c for k, c in _codes_of(section, rows).items() if any(x > 0 for x in c)}
        if refused:
            for k, c in refused.items():
                print(f"refused ({section}): {k} -> {c}")
            raise SystemExit(f"{len(refused)} rows attempted a launch: take them out of the generator")
        table[section] = rows
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write(_dump(_pack(json.loads(json.dumps(table)))) + "\n")
    n = sum(len(v) for k, v in table.items() if k != "workspace") + 2 * len(table["workspace"]["sow_workspace_bytes"]) + \
        len(table["workspace"]["small"])
    print(f"recorded {n} rows, version {lib.sow_version()}, {os.path.getsize(FIXTURE)} bytes -> {FIXTURE}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit("usage: python tests/test_host_dispatch_table_cpu.py --record")
    record()
