"""Run one case of the C ABI while other work loads the chip, bit for bit against its quiet run (a helper module, like
graph_replay.py).

Every other GPU test launches one call on an idle chip and waits.  The library does not run like that: prepare.accumulate
spreads layers over side streams, a two-stream backward runs a block's weight gradients beside the next block's data
gradients.  The streaming kernels order their LDS rings by hand (counted s_waitcnt vmcnt, raw s_barrier, inline-asm ds_read):
a wait that is one group too lax gives right answers as long as the loads land early, which on an idle chip they do.  The
kernels are deterministic by construction (fixed reduction orders, no float atomics), so the allowed difference between a
quiet and a loaded run is zero.

`prepare(b)`: the quiet run of a graph_replay.Bound on the current stream.
  * I1 loaded, outputs and workspaces 0xFF, call: return codes 0, guards intact, snapshot Q;
  * the same over zeroed outputs and workspaces: bit-identical to Q, and checked against float64 by the case's own comparator
    (the comparators read the buffers as graph_replay's second replay leaves them: zero-filled before the call);
  * the call timed with events, five times after three untimed ones (the chip idles through the float64 check); the refill
    (restore the accumulated-onto values, fill the rest) timed once.

`under_load(b, quiet, loads, reps)`: for each load and repetition
  * the load starts on its own stream: an origin event, its first kernel, an event;
  * the current stream waits on that event, refills (0xFF on even repetitions, 0x00 on odd ones) and calls, between two events;
  * the rest of the load is queued, then an end event behind its last kernel;
  * after a synchronize: return codes 0, guards intact, the snapshot equals Q bit for bit, the load's own results are intact
    (the twin's outputs equal ITS quiet snapshot), and the call ran inside the load: measured from the origin event, the call
    started no earlier than the load's first kernel ended and ended before the load's last kernel did.  A repetition that was
    not overlapped raises NotOverlapped -- never skipped, never repeated.
A load lasts at least max(30 x the quiet call (the twin: 10 x), 2 ms) plus four refills, by its own quiet pass time: it has to
outlast the loaded call, and the stream slows one kernel 10 x.

The loads are bounded sequences of ordinary kernels; none waits on a flag:
  StreamLoad   read + write elementwise passes over two 384 MiB buffers (three times the 256 MiB Infinity Cache): HBM saturation;
  GatherLoad   index_select of 2^17 seeded random 1 KiB rows out of a 1 GiB table into a fixed output: scattered long-latency reads;
  TwinLoad     another case of the plan, with its own Bound, called over and over on a second stream: two library calls in
               flight at once, which also holds the "keeps no state" contract of include/sow_amd.h under true concurrency.
               All its calls are queued before the case's call (behind a few filler passes that cover the host's queueing time),
               each between two events: a refill or call of the twin must intersect the case's call, and a call itself
               whenever the case's call is too long to fit into a refill of the twin.
Two streams are in flight at any time (the machines give four hardware queues).
"""
import math
import statistics
import time

import torch

import graph_replay as GR

DEV = "cuda"
MIN_LOAD_MS = 2.0
# A load has to outlast the LOADED call.  The stream and the gathers slow a call by up to 10.2 x (colsum_kernel, the other rows
# of profiles/under_load.txt stay under 8.2 x), so they are sized for 30 x the quiet call; beside a twin no call ran more than
# 2.6 x slower: 10 x.
LOAD_FACTOR = {"stream": 30.0, "gather": 30.0, "twin": 10.0}
REPS = 6


class NotOverlapped(AssertionError):
    """The call did not run inside its load: the repetition proves nothing about contention."""


class Quiet:
    def __init__(self, snapshot, times_ms, refill_ms, host_ms):
        self.Q, self.times, self.refill_ms, self.host_ms = snapshot, sorted(times_ms), refill_ms, host_ms
        self.ms = statistics.median(times_ms)

    @property
    def spread(self):
        """max / min of the five quiet timings."""
        return self.times[-1] / max(self.times[0], 1e-6)


def _ev():
    return torch.cuda.Event(enable_timing=True)


def _called(rc, name, what):
    bad = rc.failed()
    assert not bad, f"{name}: {what}: " + ", ".join(f"{w} returned {c}" for w, c in bad)


def prepare(b, trace=None, timings=5):
    import test_gpu_elementwise as E
    rc = GR.Rc()
    cur = torch.cuda.current_stream()
    b.load(0)
    b.fill(0xFF)
    if trace is not None:
        trace.extend(E._kernel_seq(lambda: b.call(rc)))
    else:
        b.call(rc)
    _called(rc, b.name, "quiet run")
    b.check_guards(f"{b.name}: quiet run")
    Q = b.snapshot()
    b.fill(0x00)
    b.call(rc)
    _called(rc, b.name, "quiet run over zeroed workspaces")
    b.check_guards(f"{b.name}: quiet run over zeroed workspaces")
    again = b.snapshot()
    GR._same(again, Q, f"{b.name}: quiet run over zeroed workspaces against the quiet run over 0xFF")
    if b.check is not None:
        b.check(0, {k: v.cpu() for k, v in again.items()})
    host = []
    for _ in range(3):         # the chip sat idle through the float64 check: three untimed calls before the timed ones
        h0 = time.perf_counter()
        b.fill(0xFF)
        b.call(rc)
        host.append(1e3 * (time.perf_counter() - h0))          # what the host takes to queue one refill and call
    times = []
    r0, r1 = _ev(), _ev()
    for k in range(timings):
        r0.record(cur)
        b.fill(0xFF)
        r1.record(cur)
        e0, e1 = _ev(), _ev()
        e0.record(cur)
        b.call(rc)
        e1.record(cur)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    _called(rc, b.name, "timed quiet runs")
    return Quiet(Q, times, r0.elapsed_time(r1), max(host))


# ------------------------------------------------------------------------------------------------------------------ loads
class _PassLoad:
    """A load made of identical passes on one stream; `pass_ms`: the quiet time of one pass (median of 5)."""
    name = ""

    def __init__(self):
        self.stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        ts = []
        with torch.cuda.stream(self.stream):
            self.one()
            for _ in range(5):
                a, z = _ev(), _ev()
                a.record(self.stream)
                self.one()
                z.record(self.stream)
                self.stream.synchronize()
                ts.append(a.elapsed_time(z))
        self.pass_ms = statistics.median(ts)

    def one(self):
        raise NotImplementedError

    def begin(self, target_ms, case_host_ms=0.0, case_ms=0.0):
        """Origin event, the first kernel, the event behind it.  Everything is queued now: the passes take far longer on
        the GPU than on the host."""
        n = int(math.ceil(target_ms / self.pass_ms)) + 1
        origin, first = _ev(), _ev()
        with torch.cuda.stream(self.stream):
            origin.record(self.stream)
            self.one()
            first.record(self.stream)
            for _ in range(n - 1):
                self.one()
        return origin, first

    def finish(self):
        last = _ev()
        last.record(self.stream)
        return last

    def verify(self, what, t_start=None, t_end=None):
        pass


class StreamLoad(_PassLoad):
    name = "stream"

    def __init__(self, mib=384):
        n = mib << 18                                   # fp32 elements
        self.src = torch.ones(n, dtype=torch.float32, device=DEV)
        self.dst = torch.empty(n, dtype=torch.float32, device=DEV)
        super().__init__()

    def one(self):
        torch.add(self.src, 1.0, out=self.dst)


class GatherLoad(_PassLoad):
    name = "gather"

    def __init__(self, rows=1 << 20, picks=1 << 17):
        self.table = torch.ones(rows, 256, dtype=torch.float32, device=DEV)          # 1 GiB of 1 KiB rows
        g = torch.Generator().manual_seed(1234)
        self.idx = torch.randint(0, rows, (picks,), generator=g).to(DEV)
        self.out = torch.empty(picks, 256, dtype=torch.float32, device=DEV)
        super().__init__()

    def one(self):
        torch.index_select(self.table, 0, self.idx, out=self.out)


class TwinLoad:
    """Another case on a second stream, refilled and called n times back to back.  Every call is queued before the case's own
    call is: the twin's stream first runs `filler` passes (a _PassLoad's, bounded like everything else) for three times as long as
    the host takes to queue the n calls and the case, so that when the first twin call starts the queues of both streams are
    full, however short the calls are.  Each twin call sits between two events: verify() asserts that at least one of them was
    in flight during the case's call."""
    name = "twin"

    def __init__(self, b, quiet, stream, filler):
        self.b, self.quiet, self.stream, self.filler = b, quiet, stream, filler
        self.rc = GR.Rc()
        self.calls = []

    def begin(self, target_ms, case_host_ms=0.0, case_ms=0.0):
        self.must_hit = case_ms > 3.0 * self.quiet.refill_ms
        n = int(math.ceil(target_ms / max(self.quiet.ms, 1e-3))) + 1
        host_ms = 3.0 * (n * (self.quiet.host_ms + 0.05) + case_host_ms) + 1.0
        origin, first = _ev(), _ev()
        self.calls = []
        with torch.cuda.stream(self.stream):
            for _ in range(int(math.ceil(host_ms / self.filler.pass_ms))):
                self.filler.one()
            origin.record(self.stream)
            for k in range(n):
                f, a, z = _ev(), _ev(), _ev()
                f.record(self.stream)
                self.b.fill(0xFF)
                a.record(self.stream)
                self.b.call(self.rc)
                z.record(self.stream)
                self.calls.append((f, a, z))
                if k == 0:
                    first.record(self.stream)
        self.origin = origin
        return origin, first

    def finish(self):
        last = _ev()
        last.record(self.stream)
        return last

    def verify(self, what, t_start=None, t_end=None):
        _called(self.rc, self.b.name, what)
        self.b.check_guards(f"{what}: the twin {self.b.name}")
        GR._same(self.b.snapshot(), self.quiet.Q, f"{what}: the twin {self.b.name} against its own quiet run")
        if t_start is None:
            return None
        # The twin's stream runs refill, call, refill, call ... without a pause, so one of its iterations is in flight during
        # the case's call.  A library call of the twin itself must be whenever the case's call cannot fit into a refill of the
        # twin: when its quiet time exceeds three quiet refills of the twin (a call beside a twin slows by up to 2.6 x).  Calls of
        # a few microseconds beside a longer refill can fall into the gap; how often they did not is reported.
        spans = [tuple(self.origin.elapsed_time(e) for e in fz) for fz in self.calls]
        direct = any(a < t_end and z > t_start for _, a, z in spans)
        some = any(f < t_end and z > t_start for f, _, z in spans)
        if not some or (self.must_hit and not direct):
            raise NotOverlapped(f"{what}: NOT OVERLAPPED -- no {'call' if some else 'refill or call'} of the {len(spans)} of the twin "
                                f"{self.b.name} (the first {spans[0][1]:.3f} .. {spans[0][2]:.3f} ms, the last {spans[-1][1]:.3f} .. "
                                f"{spans[-1][2]:.3f} ms) was in flight during the call ({t_start:.3f} .. {t_end:.3f} ms)")
        return direct


def bound_bytes(b):
    """Bytes of device memory the buffers of a Bound hold: inputs, outputs with their guards, workspaces, in-place operands."""
    seen = {}
    ts = [dst for dst, _ in b.slots] + [buf for ar in b.arenas for buf, *_ in ar.outs] + [t for t, _ in b.extras] + list(b.keep)
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            st = t.untyped_storage()
            seen[st.data_ptr()] = st.nbytes()
    return sum(seen.values())


def under_load(b, quiet, loads, reps=REPS):
    """The loaded repetitions of the module docstring.  Returns {load name: [loaded call time in ms per repetition]}."""
    cur = torch.cuda.current_stream()
    report = {"twin_calls_hit": 0}
    for load in loads:
        target = max(LOAD_FACTOR[load.name] * quiet.ms, MIN_LOAD_MS) + 4.0 * quiet.refill_ms
        rows = report[load.name] = []
        for rep in range(reps):
            what = f"{b.name}: under {load.name}, repetition {rep}"
            rc = GR.Rc()
            torch.cuda.synchronize()
            origin, first = load.begin(target, quiet.host_ms, quiet.ms)
            cur.wait_event(first)
            b.fill(0xFF if rep % 2 == 0 else 0x00)
            e0, e1 = _ev(), _ev()
            e0.record(cur)
            b.call(rc)
            e1.record(cur)
            last = load.finish()
            torch.cuda.synchronize()
            _called(rc, b.name, what)
            b.check_guards(what)
            GR._same(b.snapshot(), quiet.Q, f"{what} against the quiet run")
            t_first, t_start, t_end, t_last = (origin.elapsed_time(e) for e in (first, e0, e1, last))
            report["twin_calls_hit"] += bool(load.verify(what, t_start, t_end))
            if not (t_start - t_first >= 0.0 and t_last - t_end > 0.0):
                raise NotOverlapped(f"{what}: NOT OVERLAPPED -- from the load's origin: its first kernel ended at {t_first:.3f} ms, "
                                    f"the call ran {t_start:.3f} .. {t_end:.3f} ms, the load's last kernel ended at {t_last:.3f} ms "
                                    f"(quiet call {quiet.ms:.3f} ms, load sized for {target:.3f} ms)")
            rows.append(e0.elapsed_time(e1))
    return report
