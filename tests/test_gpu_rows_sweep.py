"""-m gpu: the seeded sweep of tests/rows_plan.py -- sow_forward_skinny_rows (33 - 64 rows, four accumulator kinds, fp32 factors)
and the short-batch pairs sow_forward_short / sow_backward_short and sow_forward_short_codes / sow_backward_short_codes (1 - 1024
rows) over the classes of their slab plans: slab length, tail and column class of either direction, slab counts past 16, rank-tile
counts 1 - 4, one to sixteen row blocks, the row-tile edges of the last block, launch-pair splits.

Nothing of the protocol is new: the runners and comparators of test_gpu_skinny_rows.py, test_gpu_short_rows.py and
test_gpu_short_codes.py are imported -- NaN neighbours around every input, sentinel guards around every output, three runs on 0xFF /
0x00 / 0xFF memory that must agree bit for bit, every element held to the float64 comparators of test_gpu_skinny._check /
test_gpu_elementwise._check on W^, and dX and dh of every case on codes bit for bit what sow_backward_short gives on the image.
No tolerance is added.  tests/test_rows_plan_cpu.py shows on the CPU that these comparators reject a result with any one of the
classes left out.

test_gpu_short_codes._dh reads dh at the front of the workspace: plan_ws (api.hip) sets off_dh = 0 before anything else, for every
shape.  The guarded code and scale buffers start 64 bytes into an allocation (test_gpu_fp8_acc._guarded_bytes), 8-byte aligned
whatever d_out is; test_codes_operands_are_aligned asserts it for the planned shapes."""
import dataclasses
import gc

import pytest
import torch

import rows_plan as RP
import skinny_sweep as SW
import test_gpu_elementwise as E
import test_gpu_short_codes as C
import test_gpu_short_rows as P
import test_gpu_skinny_rows as RW
from sow_amd import _lib

pytestmark = pytest.mark.gpu
PLAN = RP.plan()
FMT = {"dense": "dense", "e4m3": "fp8", "mxfp4": "fp4", "none": "none"}
WORST = {"rows": {}, "short": {}, "short_codes": {}, "short_groups": {}}     # family -> {case or (case, stage): err / bound}


def _name(c):
    return c.name


@pytest.fixture(autouse=True)
def _drop_cached_operands():
    """No planned case is built twice, so nothing is kept of one: the two _operands keep every layer they ever built (lru_cache),
    which here would be 130 layers and their accumulators, held until the process ends."""
    yield
    P._operands.cache_clear()
    C._operands.cache_clear()


@pytest.fixture(scope="module", autouse=True)
def _give_back_device_memory():
    """The module leaves the process as it found it: its device blocks (accumulators of up to 25 M elements, their partials) go
    back to the driver, and the cyclic garbage of its 118 tests (about 18 000 objects) is collected here.  Left to the collector,
    that garbage brings on a full collection somewhere in the modules that follow, and a full collection over the 0.6 M objects of
    the suite's process stops the host for about 0.3 s: longer than the filler passes of tests/under_load.py cover while
    the host queues a twin's calls, so a repetition there that meets one is not overlapped and fails."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _record(family, case, name):
    """The err / bound ratios test_gpu_elementwise._check recorded for `case`, under `family` and the planned case's name."""
    for (key, stage), v in E.WORST.items():
        if key == case.name:
            WORST[family][(name, stage)] = v[0]


# ---- sow_forward_skinny_rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PLAN.rows, ids=_name)
def test_rows(c):
    lib = _lib.load()
    dtype, fmt = RW.DT[c.dtype], FMT[c.kind]
    assert lib.sow_forward_skinny_rows_workspace_bytes(c.T, c.d_in, c.d_out, c.r, RW.KIND[fmt], E._dt(dtype)) == \
        RP.rows_ws_bytes(c.T, c.d_in, c.d_out, c.r, c.kind)
    d = RW._layer(fmt, dtype, c.T, c.d_in, c.d_out, c.r, c.bias, c.s, seed=c.seed)
    (y,) = RW._run(dtype, [d], what=c.name)
    WORST["rows"][c.name] = RW._check(c.name, dtype, d, y)["worst"]
    if c.f32:   # fp32 masters that round to the factors: the flagged call is bit for bit the call on the rounded factors
        masters = {k: SW.fp32_master(d[k]) for k in ("A", "B", "bias") if d[k] is not None}
        assert all(bool((v.to(dtype).float() != v).any()) for v in masters.values() if v.numel() >= 4), "the fp32 factors must need rounding"
        (got,) = RW._run(dtype, [dict(d, **masters)], flagged=True, what=c.name + " flagged")
        RW._same(got, y, f"{c.name}: fp32 factors against pre-rounded")


# ---- the short pairs ---------------------------------------------------------------------------------------------------------------------
def _short_layer(c):
    """(Case, operands) of a planned short case by the runner of its format."""
    if c.kind == "dense":
        return P._operands(c.dtype, c.T, c.d_in, c.d_out, c.r, c.bias, c.s, c.seed)
    return C._operands(FMT[c.kind], c.dtype, c.T, c.d_in, c.d_out, c.r, c.bias, c.s, c.seed)


def _queries_match(c):
    lib = _lib.load()
    dt = E._dt(P.DT[c.dtype])
    base = lib.sow_workspace_bytes(c.T, c.d_in, c.d_out, c.r, 0, _lib.ACC_DENSE, dt)
    if c.kind == "dense":
        assert lib.sow_forward_short_workspace_bytes(c.T, c.d_in, c.d_out, c.r, _lib.ACC_DENSE, dt) == RP.forward_short_ws_bytes(c.T, c.d_in, c.d_out, c.r)
        assert lib.sow_short_workspace_bytes(c.T, c.d_in, c.d_out, c.r, _lib.ACC_DENSE, dt) == RP.short_ws_bytes(c.T, c.d_in, c.d_out, c.r, base)
    else:
        kind = C.KIND[FMT[c.kind]]
        assert lib.sow_forward_short_codes_workspace_bytes(c.T, c.d_in, c.d_out, c.r, kind, dt) == RP.forward_short_codes_ws_bytes(c.T, c.d_in, c.d_out, c.r, c.kind)
        assert lib.sow_short_codes_workspace_bytes(c.T, c.d_in, c.d_out, c.r, kind, dt) == RP.short_codes_ws_bytes(c.T, c.d_in, c.d_out, c.r, c.kind, base)


@pytest.mark.parametrize("c", PLAN.short, ids=_name)
def test_short(c):
    _queries_match(c)
    case, d = _short_layer(c)
    (out,) = P._run([(case, d)], what=c.name)
    E._check(case, d, out)
    _record("short", case, c.name)


@pytest.mark.parametrize("c", PLAN.short_codes, ids=_name)
def test_short_codes(c):
    _queries_match(c)
    case, d = _short_layer(c)
    (out,) = C._run([(case, d)], what=c.name)
    C._check(case, d, out)
    _record("short_codes", case, c.name)
    C._identical_to_the_image([(case, d)], [out], c.name)


def test_codes_operands_are_aligned():
    """The code and scale buffers as the runners pass them, at every planned d_out: 8-byte aligned (the new entry points read the
    E4M3 exponents and the MXFP4 codes and scales in 8-byte pieces and refuse anything else)."""
    for c in PLAN.short_codes + [m for g in PLAN.short_groups if g.kind != "dense" for m in g.layers]:
        fill = RW.GUARD_BYTES[FMT[c.kind]]
        q = torch.zeros((c.d_in // (2 if c.kind == "mxfp4" else 1), c.d_out), dtype=torch.uint8, device="cuda")
        e = torch.zeros((c.d_in // 32, c.d_out) if c.kind == "mxfp4" else (c.d_out,), dtype=torch.uint8 if c.kind == "mxfp4" else torch.int8, device="cuda")
        assert RW.F8._guarded_bytes(q, fill[0]).data_ptr() % 8 == 0 and RW.F8._guarded_bytes(e, fill[1]).data_ptr() % 8 == 0, c.name


# ---- grouped calls -------------------------------------------------------------------------------------------------------------------------
IDLE_ROWS = 64     # rows the outputs of a T = 0 layer are allocated with; its x and dY hold that many rows of finite numbers


def _group_layers(g):
    """(Case, operands) per layer.  A T = 0 layer: the operands of IDLE_ROWS rows under a Case of no rows ("rows": the runners
    allocate its outputs with that many rows and hold all of them, the guards and the workspace to their fill).  share_w: the
    later layers take the first one's accumulator, as the files of either format do it."""
    out = []
    for c in g.layers:
        case, d = _short_layer(c if c.T else dataclasses.replace(c, T=IDLE_ROWS))
        if c.T == 0:
            case, d = dataclasses.replace(case, name=c.name, T=0), dict(d, rows=IDLE_ROWS)
        if g.share_w and out:
            first = out[0][1]
            if g.kind == "dense":      # cleared of ties again under the W it is run with
                d, _ = P._off_ties(case.dtype, dict(d, W=first["W"]), case.s)
            else:
                d = dict(d, W=first["W"], q=first["q"], e=first["e"])
        out.append((case, d))
    return out


@pytest.mark.parametrize("g", PLAN.short_groups, ids=_name)
def test_short_group(g):
    """One call over the layers of the group: every output of a layer is bit for bit what its call alone gives, and meets float64;
    a T = 0 layer is skipped with every byte of its outputs and its workspace left as it was filled."""
    mod = P if g.kind == "dense" else C
    keys = ("y", "h", "dx", "dA", "dB", "dbias") + (("dh",) if g.kind != "dense" else ())
    layers = _group_layers(g)
    assert sum(RP.cdiv(c.T, 64) for c, _ in layers) == g.entries()
    grouped = mod._run(layers, share_w=g.share_w, what=g.name)
    live = [(i, L, o) for i, (L, o) in enumerate(zip(layers, grouped)) if L[0].T]
    for i, L, o in live:
        (s,) = mod._run([L], runs=(0xFF,), what=f"{g.name} single {i}")
        P._same_outs(o, s, f"{g.name} layer {i}", keys=keys)
        (C._check if g.kind != "dense" else E._check)(L[0], L[1], o)
        _record("short_groups", L[0], g.layers[i].name)
    if g.kind != "dense":
        C._identical_to_the_image([L for _, L, _ in live], [o for _, _, o in live], g.name)


def test_zz_report_worst_ratios():
    for family, worst in WORST.items():
        print(f"{family}: {len(worst)} ratios")
        for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:10]:
            print(f"  {k}: worst err / bound {v:.3f}")
        assert all(v <= 1.0 for v in worst.values()), family
