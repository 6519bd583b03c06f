"""-m gpu: sow_forward_short_codes + sow_backward_short_codes + the weight phases of sow_backward_ex under HIP graph capture with
in-place replay (the protocol of tests/graph_replay.py, as tests/test_gpu_short_rows_graph.py): replays on x, dY, factors, bias,
CODES and SCALES changed in place equal the eager twins bit for bit, with the workspace poisoned, zeroed and left over.

The cases run in a process of their own, for the stream-pool reason of tests/test_gpu_skinny_rows_graph.py.  The
suite's process starts one pytest on this file (SOW_AMD_SHORT_CODES_GRAPH_INNER=1, under a time limit), reads its junit report and
gives every case the verdict of the case of the same id there."""
import os
import subprocess
import sys
import tempfile
import xml.etree.ElementTree as ET

import pytest

import graph_replay as GR
import test_gpu_elementwise as E
import test_gpu_short_codes as SC
from sow_amd import _lib

pytestmark = pytest.mark.gpu
INNER = os.environ.get("SOW_AMD_SHORT_CODES_GRAPH_INNER") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verdict():
    """None in the inner process (the case runs).  In the suite's process: a function that takes a case's request and raises
    what the same case raised in the inner process."""
    if INNER:
        yield None
        return
    with tempfile.TemporaryDirectory() as tmp:
        report = os.path.join(tmp, "inner.xml")
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-s", "-p", "no:cacheprovider", "--junitxml", report]
        try:
            run = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, SOW_AMD_SHORT_CODES_GRAPH_INNER="1"), capture_output=True, text=True, timeout=300)
            out, rc = run.stdout[-6000:] + run.stderr[-2000:], run.returncode
        except subprocess.TimeoutExpired as e:
            out, rc = f"the inner run did not end within 300 s\n{(e.stdout or b'')[-4000:]}", None
        cases = {}
        if os.path.exists(report):
            for tc in ET.parse(report).getroot().iter("testcase"):
                bad = [c for c in tc if c.tag in ("failure", "error", "skipped")]
                cases[tc.get("name")] = "\n".join(f"{c.tag}: {c.get('message')}\n{c.text}" for c in bad) if bad else None

    def give(request):
        name = request.node.name
        assert name in cases, f"{name} did not run in the inner process (exit code {rc}):\n{out}"
        assert cases[name] is None, f"{name} in the inner process:\n{cases[name]}"

    yield give


def _bound(fmt, dt, T, d_in, d_out, r, name):
    """One layer through the C ABI with two input sets (the second: other operands, other codes and scales, x and dY halved)."""
    lib = _lib.load()
    sets = []
    for k in (0, 1):
        c, d = SC._operands(fmt, dt, T, d_in, d_out, r, True, 0.5, 60 + 7 * k)
        sets.append(dict(d, x=d["x"] * 0.5, dy=d["dy"] * 0.5) if k else d)
    assert not bool((sets[0]["q"] == sets[1]["q"]).all()), "the second set holds other codes"
    c = SC._operands(fmt, dt, T, d_in, d_out, r, True, 0.5, 60)[0]
    dtype, code, kind = c.dtype, E._dt(c.dtype), SC.KIND[fmt]
    b = GR.Bound(name)
    ar = b.arena(dtype)
    x, A, B, bias, dy = (b.input(ar, (sets[0][k], sets[1][k])) for k in ("x", "A", "B", "bias", "dy"))
    # codes and scales between guards of NaN codes / NaN scale bytes, changed in place between replays like every other input
    W, sc = (SC.RW.F8._guarded_bytes(sets[0][k].to(SC.DEV), g) for k, g in zip(("q", "e"), SC.RW.GUARD_BYTES[fmt]))
    b.slots += [(W, (sets[0]["q"], sets[1]["q"])), (sc, (sets[0]["e"], sets[1]["e"]))]
    y, h, dx = b.output(ar, "y", (T, d_out)), b.output(ar, "h", (T, 64)), b.output(ar, "dx", (T, d_in))
    dA, dB, dbias = b.output(ar, "dA", (d_in, r)), b.output(ar, "dB", (r, d_out)), b.output(ar, "dbias", (d_out,))
    ws = b.workspace(ar, lib.sow_short_codes_workspace_bytes(T, d_in, d_out, r, kind, code))
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y, a.h_save, a.dy, a.dx = (E._ptr(t) for t in (x, A, B, W, sc, bias, y, h, dy, dx))
    a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, kind, 0.5
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    b.keep += [arr, W, sc]

    def call(rc):
        st = E._stream()
        rc(lib.sow_forward_short_codes(arr, 1, code, st), "sow_forward_short_codes")
        rc(lib.sow_backward_short_codes(arr, 1, code, st), "sow_backward_short_codes")
        rc(lib.sow_backward_ex(E._ptr(dy), E._ptr(x), E._ptr(h), E._ptr(A), E._ptr(B), E._ptr(W), None, E._ptr(dx), E._ptr(dA), E._ptr(dB),
                               E._ptr(dbias), T, d_in, d_out, r, 0, _lib.ACC_DENSE, 0.5, 0.0, code, ws.data_ptr(), ws.numel(),
                               _lib.BWD_WEIGHTS, st), "sow_backward_ex")

    b.call = call
    case1 = E.Case(name + "_I2", dtype, T, d_in, d_out, r, acc="dense", bias=True, s=0.5)
    b.check = lambda k, out: SC._check(case1, sets[k], out)
    return b


@pytest.mark.parametrize("fmt,dt,T,d_in,d_out,r", [("fp8", "bf16", 100, 264, 520, 50), ("fp4", "f16", 129, 544, 264, 8)], ids=lambda v: str(v))
def test_graph_replay_forward_data_weights(fmt, dt, T, d_in, d_out, r, request, verdict):
    if verdict is not None:
        return verdict(request)
    b = _bound(fmt, dt, T, d_in, d_out, r, f"graph_short_codes_{fmt}_{dt}_{T}")
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "skinny_a_kernel") and GR.has_kernel(trace, "skinny_b_kernel"), sorted(set(trace))
