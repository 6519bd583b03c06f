"""-m gpu: every kernel family at the smallest shape whose LDS rings wrap, run while other work loads the chip, bit for bit
against its quiet run.

The cases are those of tests/race_plan.py (ring-wrap and multi-block shapes for the kernels that order their LDS rings by hand,
the graph_plan case for every other kernel), the buffers and float64 comparators those of tests/test_gpu_graph_replay.py
(BUILDERS, unchanged), the protocol that of tests/under_load.py: a quiet run that passes its family's own comparator, then six
repetitions under each of three loads -- an HBM-saturating stream, scattered row gathers, and the next case of the plan on a
second stream -- every one proved by events to have run inside its load and bit-identical to the quiet run.  No tolerance is
introduced here.  The quiet run of every case is traced; test_zz_under_load_report (last) asserts that every kernel the plan
claims appeared, that claims cover every __global__ of the sources, and prints one row per case (profiles/under_load.txt).

test_two_stream_backward_schedule and test_accumulate_on_side_streams hold the two places where the library itself puts
kernels of different calls in flight together (bench.Stack.backward_all(streams=2), prepare._accumulate_layers) to the result
of the same work on one stream.
"""
import statistics
import time

import pytest
import torch

import graph_replay as GR
import race_plan as RP
import test_gpu_elementwise as E
import test_gpu_graph_replay as G
import under_load as UL
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
READY = {}                   # (case id, switches) -> (Bound, Quiet, trace): the case under test and its twin, kept for the next test
REPORT = {}                  # case id -> row of the report
STARTED = []


@pytest.fixture(scope="module")
def loads():
    STARTED.append(time.time())
    yield [UL.StreamLoad(), UL.GatherLoad()], torch.cuda.Stream()
    READY.clear()


def _twin_of(case):
    """The next case of the plan.  It is built and run under the switch table of the case under test: the table is the one piece
    of state the library keeps, and two calls in flight share it."""
    return RP.CASES[(RP.CASES.index(case) + 1) % len(RP.CASES)]


def _ready(case, sw):
    key = (case.id, tuple(sorted(sw.items())))
    if key not in READY:
        trace = []
        b = G.BUILDERS[case.kind](case)
        READY[key] = (b, UL.prepare(b, trace), trace)
    return READY[key]


@pytest.mark.parametrize("case", RP.CASES, ids=lambda c: c.id)
def test_under_load(case, loads):
    passes, twin_stream = loads
    twin = _twin_of(case)
    sw = RP.switches(case)
    for key in [k for k in READY if k[0] not in (case.id, twin.id)]:
        del READY[key]                                   # two cases resident at a time
    with _lib.switch(**sw):                              # the workspace plans and the dispatch both read the switches
        b, quiet, trace = _ready(case, sw)
        missing = [k for k in case.claims if not GR.has_kernel(trace, k)]
        assert not missing, f"{case.id}: claims {missing}, the quiet trace holds {sorted(set(trace))}"
        tb, tquiet, _ = _ready(twin, sw)
        for bb in (b, tb):       # the size cap of the plan, held on what the Bound really allocated
            assert UL.bound_bytes(bb) <= RP.MAX_BYTES, f"{bb.name}: {UL.bound_bytes(bb) / 2 ** 20:.0f} MiB of buffers"
        rep = UL.under_load(b, quiet, passes + [UL.TwinLoad(tb, tquiet, twin_stream, passes[0])])
    REPORT[case.id] = dict(kernels=case.claims, quiet_ms=quiet.ms, spread=quiet.spread, loaded=rep, twin=twin.id, trace=trace)


# ------------------------------------------------------------------------------------------------ two-stream backward
DENSE_IN, DENSE_OUT = 712, 520      # gemm3s with the rank extension: 12 stages of 64 k forward (the last of 8), 9 backward


def _block_layers(seed):
    """Two layers of a "block" at ring-wrap shapes: one on chain2, one with a dense accumulator on the fused product (both
    directions pass the bf16 gate of pick_gemm, so y and dX are rounded once: the rule of fuzz_plan.py)."""
    import fuzz_plan as FP
    assert FP.gemm2_ok(RP.TW, DENSE_OUT, DENSE_IN) and FP.gemm2_ok(RP.TW, DENSE_IN, DENSE_OUT)
    return [E.Case(f"two_stream.b{seed}.chain2", BF16, RP.TW, RP.W, RP.W, 50, bias=True, s=0.5, seed=10 * seed),
            E.Case(f"two_stream.b{seed}.dense", BF16, RP.TW, DENSE_IN, DENSE_OUT, 16, acc="dense", bias=False, s=1.0,
                   seed=10 * seed + 1)]


def test_two_stream_backward_schedule():
    """Three blocks of two layers through ops.LayerGroup on the schedule of bench.Stack.backward_all(streams=2): BWD_DATA of a
    block on the main stream, side.wait_stream(main), the block's BWD_WEIGHTS_PARTIAL | BWD_GROUP_SLABS on the side stream while
    the main stream goes on to the next block, main.wait_stream(side) and ONE deferred reduction at the end.  Bit-identical to
    the same schedule on one stream; y, h, dX, dA, dB, dbias of every layer within the layer comparator (E._check)."""
    from sow_amd import ops
    blocks = [_block_layers(k) for k in range(3)]
    data, calls, outs, groups = [], [], [], []
    for layers in blocks:
        cs = []
        for c in layers:
            d = E._inputs(c)
            dev = {k: (None if v is None else v.to(DEV)) for k, v in d.items()}
            o = dict(y=torch.empty(c.T, c.d_out, dtype=c.dtype, device=DEV), h=torch.empty(c.T * 64, dtype=c.dtype, device=DEV),
                     dx=torch.empty(c.T, c.d_in, dtype=c.dtype, device=DEV), dA=torch.empty(c.d_in, c.r, dtype=c.dtype, device=DEV),
                     dB=torch.empty(c.r, c.d_out, dtype=c.dtype, device=DEV),
                     dbias=torch.empty(c.d_out, dtype=c.dtype, device=DEV) if c.bias else None)
            kind = _lib.ACC_DENSE if c.acc == "dense" else _lib.ACC_NONE
            ws = torch.empty(ops.workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, kind, c.dtype) + 256, dtype=torch.uint8, device=DEV)
            cs.append(ops.LayerCall(dev["x"], dev["A"], dev["B"], acc_down=dev.get("W"), bias=dev["bias"], scale=c.s, y=o["y"],
                                    h=o["h"], dy2=dev["dy"], dx=o["dx"], out=(o["dA"], o["dB"], o["dbias"]), grad_beta=0.0,
                                    workspace=ws))
            data.append((c, d, dev))
            outs.append(dict(o, ws=ws))
        calls.append(cs)
        groups.append(ops.LayerGroup(cs))
    tn_ph = _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS
    side = torch.cuda.Stream()

    def poison(byte):
        for o in outs:
            for t in o.values():
                if t is not None:
                    t.view(torch.uint8).fill_(byte)

    filler = torch.ones(96 << 20, dtype=F32, device=DEV)        # 384 MiB: a pass over it gives the host time to queue the step
    spans = []

    def ev(stream):
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def step(two_streams):
        red = ops.DeferredReduce()
        main = torch.cuda.current_stream()
        for _ in range(8):                           # both queues are full before the first kernel of the step starts
            filler.add_(1.0)
        for g in groups:
            g.forward()
        del spans[:]
        for g in reversed(groups):
            d0 = ev(main)
            g.backward(_lib.BWD_DATA)
            d1 = ev(main)
            if two_streams:
                side.wait_stream(main)               # after this block's data-gradient kernels (they produce dh)
                with torch.cuda.stream(side):
                    w0 = ev(side)
                    g.backward(tn_ph)
                    w1 = ev(side)
            else:
                w0 = ev(main)
                g.backward(tn_ph)
                w1 = ev(main)
            spans.append((d0, d1, w0, w1))
            red.add_group(g, tn_ph)
        if two_streams:
            main.wait_stream(side)
        red.run()
        torch.cuda.synchronize()
        return [{k: GR.bits(t).clone() for k, t in o.items() if t is not None and k != "ws"} for o in outs]

    def overlapped():
        """Blocks whose weight-gradient launch (side stream) was in flight during the NEXT block's data-gradient kernels."""
        t0 = spans[0][0]
        at = [tuple(t0.elapsed_time(e) for e in sp) for sp in spans]
        return [k for k in range(len(at) - 1) if at[k][2] < at[k + 1][1] and at[k][3] > at[k + 1][0]], at

    # the kernels of the schedule: chain2 for the first layer of a block, the fused streaming product (gemm3s with the rank
    # extension, 99 tiles of 256 x 256) for the dense one, the grouped wide weight-gradient kernel, one batched reduction
    poison(0xFF)
    trace = E._kernel_seq(lambda: step(False))
    for k in ("chain2_kernel", "gemm3s_kernel", "tn_partial_dma_wide_kernel", "tn_reduce_batch_kernel"):
        assert GR.has_kernel(trace, k), f"the schedule did not run {k}: {sorted(set(trace))}"

    poison(0xFF)
    one = step(False)
    for rep, byte in enumerate((0x00, 0xFF, 0x00)):
        poison(byte)
        two = step(True)
        both, at = overlapped()
        assert len(both) == len(blocks) - 1, (f"repetition {rep}: the weight gradients of blocks {sorted(set(range(len(blocks) - 1)) - set(both))} "
                                             f"(backward order) did not overlap the next block's data gradients; (data start, data end, "
                                             f"weights start, weights end) in ms: {[tuple(round(v, 3) for v in a) for a in at]}")
        for (c, _, _), a, e in zip(data, two, one):
            for k in e:
                diff = a[k] != e[k]
                assert not bool(diff.any()), (f"{c.name}: {k} of the two-stream schedule (repetition {rep}) differs from the "
                                              f"one-stream schedule in {int(diff.sum())} of {diff.numel()} elements")
    for (c, d, _), o in zip(data, outs):
        E._check(c, d, dict(y=o["y"].cpu(), h=o["h"].view(c.T, 64).cpu(), dx=o["dx"].cpu(), dA=o["dA"].cpu(), dB=o["dB"].cpu(),
                            dbias=None if o["dbias"] is None else o["dbias"].cpu()))


# ------------------------------------------------------------------------------------------------ accumulate on side streams
ACC_SHAPES = ((96, 160, 8), (200, 136, 16))


def _acc_model(n):
    """n SoWLinear layers on the per-layer path of prepare.accumulate (virtual_rank < min(in, out): a low-rank accumulator after
    the first round), both init methods, two shapes; factors and every later Gaussian draw fixed by seeded CPU tensors."""
    from sow_amd import SoWLinear
    net = torch.nn.ModuleList()
    for i in range(n):
        d_in, d_out, r = ACC_SHAPES[i % 2]
        m = SoWLinear(d_in, d_out, bias=False, rank=r, init_method=("normal_QR", "normal")[(i // 2) % 2], scale=0.5, device=DEV,
                      dtype=BF16)
        g = torch.Generator().manual_seed(500 + i)
        with torch.no_grad():
            m.downscale_weights[0].copy_((torch.randn(d_in, r, generator=g) * 0.05).to(BF16))
            m.upscale_weights[0].copy_((torch.randn(r, d_out, generator=g) * 0.05).to(BF16))
        m._fresh_gaussian = (lambda shape, device, dtype, g=g: (torch.randn(shape, generator=g) * 0.02).to(device, dtype))
        m._draws = g
        net.append(m)
    return net


def _acc_state(net):
    torch.cuda.synchronize()
    return [(GR.bits(m.acc_downweight.data).clone(), GR.bits(m.acc_upweight.data).clone() if m.acc_upweight.numel() else None,
             GR.bits(m.downscale_weights[0].data).clone(), GR.bits(m.upscale_weights[0].data).clone(), m.virtual_rank) for m in net]


def test_accumulate_on_side_streams():
    """prepare.accumulate spreads the per-layer accumulate() of 2 * _ACC_WIDTH + 1 layers over its side streams (QR panels, GEMMs
    and zeroing kernels of different layers in flight together; the second round reuses blocks the caching allocator got back
    from side streams); fresh identical layers run m.accumulate() one by one on the current stream.  Accumulators, factors and
    virtual_rank are bit-identical after each of two rounds, and so is the forward between them."""
    from sow_amd import prepare
    n = 2 * prepare._ACC_WIDTH + 1
    nets = [_acc_model(n), _acc_model(n)]
    assert not any(prepare._batchable(m) for m in nets[0]), "the layers must take the per-layer path"
    prepare._batchable_cached.clear()
    xs = [torch.randn(64, ACC_SHAPES[i % 2][0], generator=torch.Generator().manual_seed(i)).to(DEV, BF16) for i in range(n)]
    for rnd in range(2):
        prepare.accumulate(nets[0])
        for m in nets[1]:
            m.accumulate()
        a, b = _acc_state(nets[0]), _acc_state(nets[1])
        for i, (sa, sb) in enumerate(zip(a, b)):
            assert sa[4] == sb[4] == ACC_SHAPES[i % 2][2] * (rnd + 2), f"round {rnd}, layer {i}: virtual_rank {sa[4]} / {sb[4]}"
            for name, ta, tb in zip(("acc_downweight", "acc_upweight", "A", "B"), sa, sb):
                assert (ta is None) == (tb is None) and (ta is None or torch.equal(ta, tb)), \
                    f"round {rnd}, layer {i}: {name} after prepare.accumulate differs from accumulate() on one stream"
        del a, b
        # a forward between the rounds (the accumulator tensors of the side streams read on the current stream), and factors
        # an optimizer would have moved: B is zero after accumulate()
        with torch.no_grad():
            for net in nets:
                ys = []
                for i, m in enumerate(net):
                    m.upscale_weights[0].copy_((torch.randn(tuple(m.upscale_weights[0].shape), generator=m._draws) * 0.05).to(BF16))
                    ys.append(m(xs[i]))
                net._ys = ys
        torch.cuda.synchronize()
        for i, (ya, yb) in enumerate(zip(nets[0]._ys, nets[1]._ys)):
            assert torch.equal(GR.bits(ya), GR.bits(yb)), f"round {rnd}, layer {i}: the forward differs"
        for net in nets:
            del net._ys


# ------------------------------------------------------------------------------------------------ report and coverage
def test_zz_under_load_report():
    """Every kernel a case claims appeared in its quiet trace, claims + exemptions cover every __global__ of the sources (the
    second half also runs without a GPU: tests/test_race_plan_cpu.py), and one row per case: the kernels, the quiet time
    (median of five, with max / min of the five), per load the median loaded time and its ratio to the quiet one, and the number of
    overlapped repetitions (every repetition that was not overlapped failed its test)."""
    if len(REPORT) < len(RP.CASES):
        pytest.skip(f"the report is written after every case ({len(REPORT)} of {len(RP.CASES)} ran)")
    seen = set()
    for case in RP.CASES:
        for k in case.claims:
            assert GR.has_kernel(REPORT[case.id]["trace"], k), f"{case.id} claims {k}"
            seen.add(k)
    names = RP.GP.kernel_names()
    left = names - seen - set(RP.EXEMPT)
    assert not left, f"kernels neither run under load nor exempt: {sorted(left)}"
    names_l = ("stream", "gather", "twin")
    print()
    print(f"{'case':78s} {'quiet us':>9s} {'max/min':>7s} " + " ".join(f"{n + ' us':>10s} {'ratio':>6s}" for n in names_l)
          + "  overlapped  twin call hit  kernels")
    total = 0
    for case in RP.CASES:
        r = REPORT[case.id]
        q_ms = r["quiet_ms"]
        cols = []
        for n in names_l:
            ms = statistics.median(r["loaded"][n])
            cols.append(f"{1e3 * ms:10.1f} {ms / q_ms:6.2f}")
            total += len(r["loaded"][n])
        done = sum(len(r["loaded"][n]) for n in names_l)
        print(f"{case.id:78s} {1e3 * q_ms:9.1f} {r['spread']:7.2f} " + " ".join(cols) + f"  {done:2d} / {3 * UL.REPS}  {r['loaded']['twin_calls_hit']} / {UL.REPS}  "
              + " ".join(r["kernels"]))
    print(f"{len(seen)} of {len(names)} kernels run under load, {len(RP.EXEMPT)} exempt; {total} loaded repetitions, every one "
          f"overlapped and bit-identical to its quiet run; {time.time() - STARTED[0]:.0f} s since the first case")
