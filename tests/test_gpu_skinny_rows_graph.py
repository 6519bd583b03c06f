"""-m gpu: sow_forward_skinny_rows under HIP graph capture with in-place replay (the protocol of tests/graph_replay.py) and
under a concurrent HBM-stream load (tests/under_load.py), with a case list of its own: T = 64 for every accumulator format
through the C ABI, and the module call inside sow_amd.skinny_rows(64).  Replays on x, factors, codes and scales changed in
place equal the eager twins bit for bit; a call overlapped by the load equals its quiet run bit for bit.

The cases run in a process of their own.  Every graph_replay.replay and every under_load load takes a stream from torch's
stream pool, whose streams are never destroyed and keep their share of the process's four hardware queues;
tests/test_gpu_under_load.py, which the suite runs after this file, needs the default stream and its three side streams on four
different queues, and with these cases in the suite's process its twin stream landed on the default stream's queue (all 62
cases NotOverlapped).  So the suite's process only starts a second pytest on this file (once, SOW_AMD_ROWS_GRAPH_INNER=1, under
a time limit), reads its junit report, and gives every case the verdict of the case of the same id there: it opens no stream,
captures nothing and allocates nothing on the GPU here."""
import os
import subprocess
import sys
import tempfile
import xml.etree.ElementTree as ET

import pytest
import torch

import graph_replay as GR
import sow_amd
import test_gpu_elementwise as E
import test_gpu_fp8_acc as F8
import test_gpu_skinny_rows as R
import test_gpu_skinny_rows_module as M
import under_load as UL
from sow_amd import _lib, ops, quantize_accumulators

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
FMTS = ["none", "dense", "fp8", "fp4"]
T, D_IN, D_OUT, RANK = 64, 544, 264, 8


INNER = os.environ.get("SOW_AMD_ROWS_GRAPH_INNER") == "1"
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
            run = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, SOW_AMD_ROWS_GRAPH_INNER="1"), capture_output=True, text=True, timeout=600)
            out, rc = run.stdout[-6000:] + run.stderr[-2000:], run.returncode
        except subprocess.TimeoutExpired as e:
            out, rc = f"the inner run did not end within 600 s\n{(e.stdout or b'')[-4000:]}", None
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


def _bound(fmt, name):
    """One T = 64 layer of format `fmt` through the C ABI, with two input sets (the second: other operands, x halved)."""
    lib = _lib.load()
    dtype = BF16
    I = [R._layer(fmt, dtype, T, D_IN, D_OUT, RANK, True, 1.0, seed=60 + 7 * k) for k in (0, 1)]
    I[1] = dict(I[1], x=I[1]["x"] * 0.5)
    I[1] = dict(R.SW.off_ties(dtype, {k: v for k, v in I[1].items() if k != "fmt"})[0], fmt=fmt)
    b = GR.Bound(name)
    ar = b.arena(dtype)
    x, A, B, bias = (b.input(ar, (I[0][k], I[1][k])) for k in ("x", "A", "B", "bias"))
    W = e = None
    if fmt == "dense":
        W = b.input(ar, (I[0]["W"], I[1]["W"]))
    elif fmt in R.GUARD_BYTES:
        gq, ge = R.GUARD_BYTES[fmt]
        W = b.extra(None, F8._guarded_bytes(I[0]["q"], gq), (I[0]["q"], I[1]["q"]))
        e8 = [I[k]["e"].view(torch.uint8) for k in (0, 1)]
        e = b.extra(None, F8._guarded_bytes(e8[0], ge), (e8[0], e8[1]))
    y = b.output(ar, "y", (T, D_OUT))
    ws = b.workspace(ar, lib.sow_forward_skinny_rows_workspace_bytes(T, D_IN, D_OUT, RANK, R.KIND[fmt], E._dt(dtype)))
    arr = (_lib.LayerArgs * 1)()
    a = arr[0]
    a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y = (E._ptr(t) for t in (x, A, B, W, e, bias, y))
    a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, D_IN, D_OUT, RANK, R.KIND[fmt], 1.0
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    b.keep.append(arr)
    b.call = lambda rc: rc(lib.sow_forward_skinny_rows(arr, 1, E._dt(dtype), E._stream()), "sow_forward_skinny_rows")
    b.check = lambda k, out: R._check(f"{name}_I{k + 1}", dtype, I[k], out["y"])
    return b


@pytest.mark.parametrize("fmt", FMTS)
def test_graph_replay_rows_entry(fmt, request, verdict):
    if verdict is not None:
        return verdict(request)
    b = _bound(fmt, f"graph_rows_{fmt}")
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "skinny_a_kernel") and GR.has_kernel(trace, "skinny_b_kernel"), sorted(set(trace))


@pytest.mark.parametrize("quant", [None, "fp8_e4m3", "mxfp4"], ids=["dense", "e4m3", "mxfp4"])
def test_graph_replay_module_call_inside_the_context(quant, request, verdict):
    """One layer's no-grad forward at T = 64 inside skinny_rows(64), captured after one eager call: replays on x -- and, for a
    quantised layer, codes and scales -- changed in place equal the eager calls of the second layer."""
    if verdict is not None:
        return verdict(request)
    dtype, d = BF16, 288
    nets = [M._layer(d, d, 16, dtype, seed=31 + k) for k in (0, 1)]
    if quant:
        for m in nets:
            holder = torch.nn.ModuleList([m])
            assert quantize_accumulators(holder, fmt=quant, strict=True) == 1
    m = nets[0]
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(T, d, generator=g).to(dtype) * s for s in (1.0, 0.5)]
    b = GR.Bound(f"graph_rows_module_{quant}")
    ar = b.arena(dtype)
    x = b.input(ar, (xs[0], xs[1]))
    for name in ("downscale_weights", "upscale_weights"):
        p = getattr(m, name)[0].data
        b.extra(None, p, tuple(getattr(n, name)[0].data.clone() for n in nets))
    b.extra(None, m.bias.data, tuple(n.bias.data.clone() for n in nets))
    raw = (lambda t: t.view(torch.uint8)) if quant else (lambda t: t)
    b.extra(None, raw(m.acc_downweight.data), tuple(raw(n.acc_downweight.data).clone() for n in nets))
    if quant:
        b.extra(None, m.acc_exponent.view(torch.uint8), tuple(n.acc_exponent.view(torch.uint8).clone() for n in nets))
    y = b.output(ar, "y", (T, d))
    calls = []

    def call(rc):
        with torch.no_grad(), sow_amd.skinny_rows(64):
            calls.append(1)
            y.copy_(m(x))

    b.call = call
    wants = []
    for k in (0, 1):
        wants.append(M._cabi(nets[k], xs[k].to(DEV)))      # (before the replay loads anything into nets[0])
    b.check = lambda k, out: R._same(out["y"], wants[k], f"replay of input set {k + 1} against the C ABI on its operands")
    trace = []
    GR.replay(b, trace)
    assert GR.has_kernel(trace, "skinny_a_kernel") and not GR.has_kernel(trace, "cast_copy_kernel"), sorted(set(trace))


@pytest.fixture(scope="module")
def stream_load(verdict):
    yield UL.StreamLoad() if verdict is None else None


@pytest.mark.parametrize("fmt", ["dense", "fp8", "fp4"])
def test_rows_entry_under_hbm_stream_load(fmt, request, verdict, stream_load):
    if verdict is not None:
        return verdict(request)
    b = _bound(fmt, f"load_rows_{fmt}")
    trace = []
    quiet = UL.prepare(b, trace)
    assert GR.has_kernel(trace, "skinny_a_kernel") and GR.has_kernel(trace, "skinny_b_kernel"), sorted(set(trace))
    rep = UL.under_load(b, quiet, [stream_load])
    assert len(rep["stream"]) == UL.REPS
    print(f"{b.name}: quiet {quiet.ms * 1e3:.1f} us, under the stream load {sorted(rep['stream'])[len(rep['stream']) // 2] * 1e3:.1f} us")
