"""-m gpu: round-3 surface -- forward without the saved projection (no-grad callers), accumulator validation on the grouped
path, FactorAdamW hyper-parameters written through param_groups, and (further down) the round's new kernels.

Tolerances: `rel_err` = max |a - b| / max |b| (relative to the largest reference magnitude, not element-wise).
"""
import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from oracle import sow_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _layer(d_in, d_out, r, dtype, bias=False, dense=False, seed=0):
    from sow_amd import SoWLinear
    torch.manual_seed(seed)
    m = SoWLinear(d_in, d_out, bias=bias, rank=r, init_method="normal", device=DEV, dtype=dtype)
    nn.init.normal_(m.downscale_weights[0], std=0.05)
    nn.init.normal_(m.upscale_weights[0], std=0.05)
    if bias:
        nn.init.normal_(m.bias, std=0.1)
    if dense:
        m.acc_downweight = nn.Parameter((torch.randn(d_in, d_out, device=DEV) * 0.02).to(dtype), requires_grad=False)
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(64, 256, 256, 8), (16384, 512, 1376, 50), (1024, 768, 3072, 8), (300, 96, 40, 5)])
@pytest.mark.parametrize("dense", [False, True])
def test_forward_without_saved_projection_is_bit_identical(shape, dtype, dense):
    """torch.no_grad() callers (eval / generate of scripts/commonsense_evaluate.py:268-287, the first pass of activation
    checkpointing) run sow_forward with h_save = NULL: same y as the training forward (bit for bit on the streaming path),
    and the oracle's."""
    T, d_in, d_out, r = shape
    m = _layer(d_in, d_out, r, dtype, bias=True, dense=dense)
    x = torch.randn(T, d_in, device=DEV).to(dtype)
    y_train = m(x.clone().requires_grad_(True)).detach()
    with torch.no_grad():
        y_eval = m(x)
    assert not y_eval.requires_grad
    if dense and r <= 64:
        # a dense accumulator takes a scratch projection buffer without grad too: the same launches as training
        assert torch.equal(y_eval, y_train)
    elif T > 8192 or T < 128:
        assert torch.equal(y_eval, y_train)
    else:
        # short inputs: with a saved projection the chain is split over K (fp32 partial sums + h_reduce), without it
        # the unsplit kernel runs -- a different summation order, same value to fp32 / bf16 rounding
        assert rel_err(y_eval.float().cpu(), y_train.float().cpu()) < (1e-2 if dtype == torch.bfloat16 else 1e-6)
    acc = m.acc_downweight.data.float().cpu() if dense else None
    y_ref = O.sow_forward(x.float().cpu(), [m.downscale_weights[0].data.float().cpu()], [m.upscale_weights[0].data.float().cpu()],
                          acc, None, 1.0, m.bias.data.float().cpu())
    assert rel_err(y_eval.float().cpu(), y_ref) < (2e-2 if dtype == torch.bfloat16 else 1e-5)


def test_no_grad_forward_allocates_no_projection_buffer():
    from sow_amd import ops
    x = torch.randn(4096, 512, device=DEV, dtype=torch.bfloat16)
    A = torch.randn(512, 50, device=DEV, dtype=torch.bfloat16) * 0.05
    B = torch.randn(50, 512, device=DEV, dtype=torch.bfloat16) * 0.05
    y1, h1 = ops.sow_forward(x, A, B, None, None, None, 1.0)
    y0, h0 = ops.sow_forward(x, A, B, None, None, None, 1.0, save_h=False)
    assert h0 is None and h1 is not None and torch.equal(y0, y1)


def test_grouped_no_grad_forward_matches_single_calls():
    """group_siblings under torch.no_grad(): q / k / v share one launch, nothing is saved, outputs bit-identical."""
    from sow_amd import group_siblings, ungroup_siblings

    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = _layer(512, 512, 50, torch.bfloat16, seed=1)
            self.k_proj = _layer(512, 512, 50, torch.bfloat16, seed=2)
            self.v_proj = _layer(512, 512, 50, torch.bfloat16, seed=3)

        def forward(self, h):
            return self.q_proj(h), self.k_proj(h), self.v_proj(h)

    net = Attn()
    x = torch.randn(128, 128, 512, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        single = net(x)
        assert group_siblings(net) == 1
        grouped = net(x)
        ungroup_siblings(net)
    for a, b in zip(single, grouped):
        assert torch.equal(a, b)


@pytest.mark.parametrize("bad", ["dtype", "shape"])
def test_grouped_path_validates_the_accumulator_like_the_single_call(bad):
    """A layer whose dense accumulator was loaded in another precision / shape (load_sow of a foreign checkpoint): the
    single call raises TypeError / ValueError; LayerCall raises the same, and a sibling group falls back to the single call
    (which raises) instead of handing a mistyped pointer to the grouped launch."""
    from sow_amd import group_siblings, ops
    x = torch.randn(16384, 512, device=DEV, dtype=torch.bfloat16)
    A = (torch.randn(512, 50, device=DEV) * 0.05).bfloat16()
    B = (torch.randn(50, 512, device=DEV) * 0.05).bfloat16()
    acc = torch.randn(512, 512, device=DEV) * 0.02 if bad == "dtype" else (torch.randn(512, 256, device=DEV) * 0.02).bfloat16()
    exc = TypeError if bad == "dtype" else ValueError
    with pytest.raises(exc):
        ops.sow_forward(x, A, B, acc, None, None, 1.0)
    with pytest.raises(exc):
        ops.LayerCall(x, A, B, acc_down=acc)

    class Mlp(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj = _layer(512, 512, 50, torch.bfloat16, seed=1)
            self.up_proj = _layer(512, 512, 50, torch.bfloat16, seed=2)

        def forward(self, h):
            return self.gate_proj(h) * self.up_proj(h)

    net = Mlp()
    net.up_proj.acc_downweight = nn.Parameter(acc, requires_grad=False)
    assert group_siblings(net) == 1
    with pytest.raises(exc):
        net(x.requires_grad_(True))


def test_factor_adamw_steps_with_the_lr_a_scheduler_wrote():
    from sow_amd.dp import FactorBucket
    from sow_amd.optimizer import FactorAdamW
    ps = [nn.Parameter(torch.randn(64, 16, device=DEV)), nn.Parameter(torch.randn(16, 64, device=DEV))]
    ref = [nn.Parameter(p.detach().clone()) for p in ps]
    bucket = FactorBucket(ps)
    opt = FactorAdamW(bucket, lr=3e-3, weight_decay=0.0)
    topt = torch.optim.AdamW(ref, lr=3e-3, weight_decay=0.0)
    for step_lr in (3e-3, 1e-3, 5e-4):
        for g in opt.param_groups:
            g["lr"] = step_lr                          # simple_train.py-style scheduler write, no read-back in between
        for g in topt.param_groups:
            g["lr"] = step_lr
        for p, q in zip(ps, ref):
            grad = torch.randn_like(q)
            p.grad.copy_(grad)
            q.grad = grad.clone()
        opt.step()
        topt.step()
        assert opt.state_dict()["lr"] == step_lr
    for p, q in zip(ps, ref):
        assert rel_err(p.data.cpu(), q.data.cpu()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------
# block-level weight gradients from the module surface (verdict r2 item 4) and the bench's launch sequence (item 7)
# ---------------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    """The seven projections of a llama decoder block with HF's attribute names and a data flow that uses all of them."""

    def __init__(self, make, h=512, inter=1376):
        super().__init__()
        self.self_attn = nn.Module()
        self.mlp = nn.Module()
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            setattr(self.self_attn, n, make(h, h))
        self.mlp.gate_proj, self.mlp.up_proj, self.mlp.down_proj = make(h, inter), make(h, inter), make(inter, h)

    def forward(self, x):
        a = self.self_attn
        x = x + a.o_proj(torch.tanh(a.q_proj(x)) * torch.tanh(a.k_proj(x)) + a.v_proj(x))
        m = self.mlp
        return x + m.down_proj(torch.tanh(m.gate_proj(x)) * m.up_proj(x))


class _Tiny(nn.Module):
    def __init__(self, make, nblk=2):
        super().__init__()
        self.layers = nn.ModuleList([_Block(make) for _ in range(nblk)])

    def forward(self, x):
        for b in self.layers:
            x = b(x)
        return x


def test_block_level_weight_gradients_from_modules_vs_oracle():
    """FactorBucket.attach() on a 2-block llama-shaped stack (r = 50, bf16, T = 8192): every layer's backward runs its data
    gradient at once and the SEVEN weight-gradient jobs of a decoder block go out as one row-owner launch (the plan is
    checked through sow_backward_group_plan).  The factor gradients are compared with the CPU ORACLE run on the same
    (bf16-rounded) weights and inputs through the same data flow -- not with the per-layer HIP path."""
    import ctypes

    from oracle_backend import OracleSoWLinear
    from sow_amd import SoWLinear, _lib
    from sow_amd.dp import FactorBucket, factor_parameters
    T, r = 8192, 50
    torch.manual_seed(11)

    def make_gpu(i, o):
        m = SoWLinear(i, o, bias=False, rank=r, init_method="normal", device=DEV, dtype=torch.bfloat16)
        nn.init.normal_(m.downscale_weights[0], std=0.04)
        nn.init.normal_(m.upscale_weights[0], std=0.04)
        return m

    net = _Tiny(make_gpu)
    ref = _Tiny(lambda i, o: OracleSoWLinear(i, o, False, r, 1.0, "normal"))
    for (_, a), (_, b) in zip(net.named_modules(), ref.named_modules()):
        if isinstance(a, SoWLinear):
            b.downscale_weights[0].data = a.downscale_weights[0].data.float().cpu()
            b.upscale_weights[0].data = a.upscale_weights[0].data.float().cpu()
    x = (torch.randn(T, 512) * 0.5).bfloat16()
    bucket = FactorBucket(factor_parameters(net))
    assert bucket.attach(net) == 14 and sorted(bucket._blocks) == ["layers.0", "layers.1"]
    assert all(b["n"] == 7 for b in bucket._blocks.values())
    bucket.zero_grad()
    net(x.to(DEV)).float().square().mean().backward()
    assert not any(b["queue"] for b in bucket._blocks.values())       # both blocks went out complete, from backward
    assert len(bucket._sinks_pending) == 14
    bucket.finalize()
    torch.cuda.synchronize()
    ref(x.float()).square().mean().backward()
    for (n, a), (_, b) in zip(net.named_modules(), ref.named_modules()):
        if isinstance(a, SoWLinear):
            for pa, pb in ((a.downscale_weights[0], b.downscale_weights[0]), (a.upscale_weights[0], b.upscale_weights[0])):
                assert rel_err(pa.grad.float().cpu(), pb.grad) < 4e-2, n
    # the plan the block launch took: one resident round of the row-owner kernel
    lib = _lib.load()
    fake = 1 << 20
    arr = (_lib.LayerArgs * 7)()
    for i, (di, do) in enumerate([(512, 512)] * 4 + [(512, 1376)] * 2 + [(1376, 512)]):
        ws = lib.sow_workspace_bytes(T, di, do, r, 0, 0, _lib.BF16)
        arr[i] = _lib.LayerArgs(x=fake, A=fake, B=fake, y=fake, h_save=fake, dy=fake, dx=fake, dA=fake, dB=fake, T=T, d_in=di,
                                d_out=do, r_live=r, r_acc=0, acc_kind=0, scale=1.0, grad_beta=1.0, workspace=fake,
                                workspace_bytes=ws + 256)
    assert lib.sow_backward_group_plan(arr, 7, _lib.BF16, _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_GROUP_SLABS,
                                       (ctypes.c_int * 14)()) == 1
    # sibling groups compose with the bucket: q/k/v and gate/up run ONE forward and ONE data-gradient launch each, the weight
    # gradients still go out per decoder block
    from sow_amd import group_siblings, ungroup_siblings
    g0 = [p.grad.clone() for p in bucket.params]
    bucket.zero_grad()
    assert group_siblings(net) == 4
    net(x.to(DEV)).float().square().mean().backward()
    assert not any(b["queue"] for b in bucket._blocks.values()) and len(bucket._sinks_pending) == 14
    bucket.finalize()
    torch.cuda.synchronize()
    ungroup_siblings(net)
    for p, g in zip(bucket.params, g0):
        assert rel_err(p.grad.float().cpu(), g.float().cpu()) < 2e-2
    # gradient accumulation: a second backward adds up (the sinks finalize their pending partials first)
    g1 = [p.grad.clone() for p in bucket.params]
    net(x.to(DEV)).float().square().mean().backward()
    bucket.finalize()
    torch.cuda.synchronize()
    for p, g in zip(bucket.params, g1):
        assert rel_err(p.grad.float().cpu(), 2 * g.float().cpu()) < 2e-2


def test_bench_launch_sequence_vs_oracle():
    """bench.py's exact per-block sequence at the full T = 32768 -- grouped forward {q,k,v} {o} {gate,up} {down}, grouped
    data gradients in reverse, ONE block-level row-owner launch with BWD_GROUP_SLABS, DeferredReduce -- on one decoder block
    of llama_60m shapes (r = 50, bf16).  y, dX (sampled rows) and dA / dB (whole) against the CPU oracle in fp32 on the same
    bf16 inputs: tolerance 2e-2 of the largest reference magnitude (bf16 outputs, 32768-term sums)."""
    import importlib.util
    import os
    import sys

    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    sys.modules["bench_mod"] = bench
    spec.loader.exec_module(bench)
    T, r = 32768, 50
    shapes = bench.layer_shapes()[:7]
    stack = bench.Stack(shapes, T, r, torch.bfloat16, torch.device(DEV), "none")
    stack.step()
    torch.cuda.synchronize()
    rows = torch.arange(0, T, 997)
    for li, (di, do) in enumerate(shapes):
        x, dy = stack.x[li].float().cpu(), stack.dy[li].float().cpu()
        A, B = stack.A[li].data.float().cpu(), stack.B[li].data.float().cpu()
        y_ref = O.sow_forward(x[rows], [A], [B], None, None, 1.0, None)
        dx_ref, dA_ref, dB_ref, _ = O.sow_backward(dy, x, [A], [B], None, None, 1.0, False)
        c = stack.calls[li]
        assert rel_err(c.y[rows.to(DEV)].float().cpu(), y_ref) < 2e-2, ("y", li)
        assert rel_err(c.dx[rows.to(DEV)].float().cpu(), dx_ref[rows]) < 2e-2, ("dx", li)
        assert rel_err(stack.A[li].grad.float().cpu(), dA_ref[0]) < 2e-2, ("dA", li)
        assert rel_err(stack.B[li].grad.float().cpu(), dB_ref[0]) < 2e-2, ("dB", li)


def test_bench_dump_outputs_holds_the_timed_step(tmp_path):
    """`bench.py --dump-outputs DIR` in a child process: the line times exactly --steps replays; DIR holds one float32 .npy
    per output of the 56 layers (y / dX on the sampled rows, dA / dB whole), within DUMP_BYTES in all, and each equals what
    the same stack computes from the same seeded inputs in this process (tolerance as above)."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys

    import numpy as np

    from conftest import ROOT
    T, out_dir = 8192, tmp_path / "dump"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--tokens", str(T),
                          "--only-headline", "--no-cpu-baseline", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == 3 and len(rec["replays"]["per_replay_ms"]) == 3
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    files = sorted(os.listdir(out_dir))
    assert len(files) == 4 * 56
    assert sum(os.path.getsize(out_dir / f) for f in files) <= bench.DUMP_BYTES
    stack = bench.Stack(bench.layer_shapes(), T, 50, torch.bfloat16, torch.device(DEV), "none")
    stack.step()
    torch.cuda.synchronize()
    want = bench.stack_outputs(stack)
    assert sorted(name + ".npy" for name in want) == files
    for name, t in want.items():
        got = np.load(out_dir / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == tuple(t.shape), name
        assert rel_err(torch.from_numpy(got), t.float().cpu()) < 2e-2, name


# ---------------------------------------------------------------------------------------------------------------
# tensor-train optimizer state through the batched entry points
# ---------------------------------------------------------------------------------------------------------------
TT_CASES = [((81, 81), [1, 4, 4, 4, 1]), ((512, 512), [1, 8, 8, 1]), ((100, 60), [1, 16, 1]), ((768, 3072), [1, 16, 1]),
            ((512, 1376), [1, 8, 8, 1]), ((37, 5), [1, 3, 1])]


def test_tt_batch_decompose_and_reconstruct_match_the_per_train_path():
    """sow_tt_decompose_batch / sow_tt_reconstruct_batch against TensorTrain.from_matrix / to_matrix (the per-train path,
    itself pinned by tests/golden/tt_*.npz): same cores (same Householder reflectors; the trailing R = Q^T L is summed in a
    different order) and the same reconstruction, for padded and unpadded shapes, orders 2-4."""
    from sow_amd.tt import TensorTrain, from_matrix_batch, to_matrix_batch
    torch.manual_seed(5)
    for shape, ranks in TT_CASES:
        mats = [torch.randn(*shape, device=DEV) * (0.5 + i) for i in range(3)]
        single = [TensorTrain.from_matrix(m, ranks=ranks, padding=True) for m in mats]
        batch = from_matrix_batch(mats, ranks)
        for a, b in zip(single, batch):
            assert [tuple(c.shape) for c in a.cores] == [tuple(c.shape) for c in b.cores]
            assert list(a.ranks) == list(b.ranks) and tuple(a.input_shape) == tuple(b.input_shape)
            for ca, cb in zip(a.cores, b.cores):
                assert rel_err(cb.cpu(), ca.cpu()) < 1e-4, (shape, ranks)
        dense_single = [t.to_matrix(shape).contiguous() for t in single]
        dense_batch = to_matrix_batch(batch, [shape] * 3)
        for a, b in zip(dense_single, dense_batch):
            assert tuple(b.shape) == tuple(shape) and rel_err(b.cpu(), a.cpu()) < 1e-4, (shape, ranks)
    # a matrix of TT rank 3 (a sum of three Kronecker products) is reproduced exactly by a rank-16 train
    low = sum(torch.kron(torch.randn(8, 8, device=DEV), torch.randn(8, 8, device=DEV)) for _ in range(3))
    tt = from_matrix_batch([low], [1, 16, 1])[0]
    assert rel_err(to_matrix_batch([tt], [(64, 64)])[0].cpu(), low.cpu()) < 1e-4


@pytest.mark.parametrize("batched", [True, False])
def test_ttadam_golden_traces_through_both_paths(batched):
    """The reference's 3-step TTAdam traces (tests/golden/tt_optim.npz, ttadam.py:68-115) through sow_ttadam_batch and
    through the per-parameter path."""
    from conftest import load_golden
    from sow_amd import TTAdam
    g = load_golden("tt_optim")
    ranks = [1, 4, 4, 4, 1]
    old = TTAdam.batched
    TTAdam.batched = batched
    try:
        for wd_name, wd in (("nowd", 0.0), ("wd", 0.1)):
            p = nn.Parameter(g[f"adam_{wd_name}_p0"].to(DEV))
            opt = TTAdam([{"params": [p], "ranks": ranks}], lr=1e-2, weight_decay=wd)
            for s in range(3):
                p.grad = g[f"adam_{wd_name}_g{s}"].to(DEV)
                opt.step()
                assert rel_err(p.data.cpu(), g[f"adam_{wd_name}_p{s + 1}"]) < 1e-4
            assert opt.state[p]["step"] == 3
            assert [tuple(c.shape) for c in opt.state[p]["exp_avg"].cores] == [(1, 3, 3, 4), (4, 3, 3, 4), (4, 3, 3, 4), (4, 3, 3, 1)]
    finally:
        TTAdam.batched = old


def test_ttadam_sixteen_parameters_batched_equals_per_parameter():
    from sow_amd import TTAdam
    torch.manual_seed(9)
    shapes = [(512, 512)] * 8 + [(512, 1376)] * 4 + [(768, 768)] * 4
    ranks = [1, 8, 8, 1]

    def run(batched):
        torch.manual_seed(10)
        ps = [nn.Parameter(torch.randn(*s, device=DEV) * 0.02) for s in shapes]
        old = TTAdam.batched
        TTAdam.batched = batched
        try:
            opt = TTAdam([{"params": ps, "ranks": ranks}], lr=1e-3, weight_decay=0.01)
            for s in range(3):
                for i, p in enumerate(ps):
                    gen = torch.Generator(device=DEV).manual_seed(100 * s + i)
                    p.grad = torch.randn(p.shape, generator=gen, device=DEV) * 1e-2
                opt.step()
        finally:
            TTAdam.batched = old
        return [p.data.clone() for p in ps], opt

    a, oa = run(True)
    b, ob = run(False)
    for x, y in zip(a, b):
        # three lossy rank-8 re-compressions of random moments: 1 / (sqrt(v) + eps) amplifies the 1e-6 differences of the
        # two summation orders where v is clamped near zero
        assert rel_err(x.cpu(), y.cpu()) < 2e-4
    pa, pb = oa.param_groups[0]["params"][0], ob.param_groups[0]["params"][0]
    ma = oa.state[pa]["exp_avg"].to_matrix((512, 512))
    mb = ob.state[pb]["exp_avg"].to_matrix((512, 512))
    assert rel_err(ma.cpu(), mb.cpu()) < 1e-3


# ---------------------------------------------------------------------------------------------
# chain3f.hip: the fp32 streaming chain with pre-split factor planes (T >= 8192)
C3F_CASES = [
    # T, d_in, d_out, r, bias, scale, acc
    (32768, 768, 768, 50, False, 1.0, None),       # BASELINE.json north_star point
    (8192, 512, 1376, 50, True, 0.5, None),
    (8200, 1376, 512, 50, False, 2.0, None),       # ragged last token block
    (8192, 260, 132, 8, True, 1.0, None),          # widths not a multiple of 64, one rank tile
    (9000, 64, 72, 33, True, 1.0, None),           # r just over one tile, ragged
    (8192, 768, 768, 64, True, 1.0, None),         # r = 64: no free ones column (dbias by column sums)
    (8192, 128, 64, 2, False, 1.0, None),
    (8192, 256, 320, 16, True, 0.25, "lowrank"),   # low-rank accumulator: second chain launch with beta = 1
    (8192, 320, 256, 50, False, 1.0, "lowrank64"), # ... a 64-wide one (both chains on two rank tiles, four k-steps)
    (8192, 768, 768, 8, True, 0.125, "dense"),     # config-4 style: fp32 dense accumulator + live rank 8
    (4100, 768, 320, 50, True, 1.0, None),         # below chain3f's threshold, above the quad kernel's: chain2f + quad, ragged T
]


@pytest.mark.parametrize("case", C3F_CASES, ids=lambda c: "T%d_%dx%d_r%d%s" % (c[0], c[1], c[2], c[3], "_" + c[6] if c[6] else ""))
def test_chain3f_fp32_vs_oracle(case):
    """fp32 forward + backward at T >= 8192 (chain3f: factor planes split once per launch, 128-token workgroups, direct
    row-segment stores) against the oracle, and against the chain2f path (NO_CHAIN3F) it replaces."""
    from sow_amd import _lib, ops
    T, d_in, d_out, r, has_bias, scale, acc = case
    gen = torch.Generator(device=DEV).manual_seed(T + d_in + r)
    x = torch.randn(T, d_in, generator=gen, device=DEV)
    dy = torch.randn(T, d_out, generator=gen, device=DEV)
    A = torch.randn(d_in, r, generator=gen, device=DEV) * 0.05
    B = torch.randn(r, d_out, generator=gen, device=DEV) * 0.05
    bias = torch.randn(d_out, generator=gen, device=DEV) * 0.1 if has_bias else None
    acc_down = acc_up = None
    if acc in ("lowrank", "lowrank64"):
        ra = 24 if acc == "lowrank" else 64
        acc_down = torch.randn(d_in, ra, generator=gen, device=DEV) * 0.05
        acc_up = torch.randn(ra, d_out, generator=gen, device=DEV) * 0.05
    elif acc == "dense":
        acc_down = torch.randn(d_in, d_out, generator=gen, device=DEV) * 0.02
    cpu = lambda t: None if t is None else t.cpu()

    def run():
        y, h = ops.sow_forward(x, A, B, acc_down, acc_up, bias, scale)
        return (y,) + tuple(ops.sow_backward(dy, x, h, A, B, acc_down, acc_up, scale, has_bias))

    new = run()
    with _lib.switch(NO_CHAIN3F=1):
        old = run()
    y_ref = O.sow_forward(x.cpu(), [A.cpu()], [B.cpu()], cpu(acc_down), cpu(acc_up), scale, cpu(bias))
    dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(dy.cpu(), x.cpu(), [A.cpu()], [B.cpu()], cpu(acc_down), cpu(acc_up), scale, has_bias)
    refs = (y_ref, dx_ref, dA_ref[0], dB_ref[0], db_ref)
    tols = (1e-5, 1e-5, 2e-5, 2e-5, 2e-5)   # weight gradients: T-term sums, summation order
    for name, got, prev, ref, tol in zip(("y", "dx", "dA", "dB", "dbias"), new, old, refs, tols):
        if ref is None:
            continue
        assert rel_err(got.cpu(), ref) < tol, name
        assert rel_err(prev.cpu(), ref) < tol, name + " (chain2f)"


# ---------------------------------------------------------------------------------------------
# gemm4 split-K: short bf16 products (config 5: T = 1024) -- fewer output tiles than CUs, K split over workgroups
@pytest.mark.parametrize("shape", [(1024, 11008, 4096), (1000, 6152, 4104), (512, 8192, 8192), (2048, 6144, 4096), (256, 16384, 512)])
@pytest.mark.parametrize("trans_b", [False, True])
def test_gemm_split_k(shape, trans_b):
    """sow_gemm_ex with scratch: fp32 partial products of the K ranges through the workspace, summed in split order by a second
    launch -- against an fp32 product of the same bf16 operands, against the unsplit kernels (NO_SPLITK), with beta / bias,
    and twice (bit-identical)."""
    from sow_amd import _lib, ops
    M, K, N = shape
    gen = torch.Generator(device=DEV).manual_seed(M + K + N)
    a = torch.randn(M, K, generator=gen, device=DEV).bfloat16()
    b = (torch.randn((N, K) if trans_b else (K, N), generator=gen, device=DEV) * 0.05).bfloat16()
    bias = (torch.randn(N, generator=gen, device=DEV) * 0.1).bfloat16()
    c0 = torch.randn(M, N, generator=gen, device=DEV).bfloat16()
    lib = _lib.load()
    assert lib.sow_gemm_workspace_bytes(M, N, K, 0, _lib.BF16) > 0, "shape expected to split"
    ref = a.float() @ (b.float().t() if trans_b else b.float())
    out = ops.gemm(a, b, trans_b=trans_b)
    out2 = ops.gemm(a, b, trans_b=trans_b)
    assert torch.equal(out, out2)
    assert rel_err(out.float().cpu(), ref.cpu()) < 1e-2
    with _lib.switch(NO_SPLITK=1):
        assert lib.sow_gemm_workspace_bytes(M, N, K, 0, _lib.BF16) == 0
        plain = ops.gemm(a, b, trans_b=trans_b)
    assert rel_err(out.float().cpu(), plain.float().cpu()) < 8e-3   # one bf16 rounding of differently ordered fp32 sums
    full = ops.gemm(a, b, trans_b=trans_b, out=c0.clone(), alpha=0.5, beta=0.25, bias=bias)
    ref2 = 0.5 * ref + 0.25 * c0.float() + bias.float()
    assert rel_err(full.float().cpu(), ref2.cpu()) < 1e-2


@pytest.mark.parametrize("shape", [(1024, 4096, 4096), (1024, 11008, 4096), (1024, 4096, 11008)])
def test_dense_layer_short_t_split_k_vs_oracle(shape):
    """The dense-accumulator layer at the config-5 shapes (llama-7b q / down / up, T = 4 x 256, r = 8, bf16): forward and
    backward through sow_forward / sow_backward (split-K scratch inside the layer workspace) against the oracle."""
    from sow_amd import ops
    T, d_in, d_out = shape
    r = 8
    gen = torch.Generator(device=DEV).manual_seed(d_in + d_out)
    x = torch.randn(T, d_in, generator=gen, device=DEV).bfloat16()
    dy = torch.randn(T, d_out, generator=gen, device=DEV).bfloat16()
    A = (torch.randn(d_in, r, generator=gen, device=DEV) * 0.05).bfloat16()
    B = (torch.randn(r, d_out, generator=gen, device=DEV) * 0.05).bfloat16()
    W = (torch.randn(d_in, d_out, generator=gen, device=DEV) * 0.02).bfloat16()
    y, h = ops.sow_forward(x, A, B, W, None, None, 0.125)
    dx, dA, dB, _ = ops.sow_backward(dy, x, h, A, B, W, None, 0.125, False)
    f = lambda t: t.float().cpu()
    y_ref = O.sow_forward(f(x), [f(A)], [f(B)], f(W), None, 0.125, None)
    dx_ref, dA_ref, dB_ref, _ = O.sow_backward(f(dy), f(x), [f(A)], [f(B)], f(W), None, 0.125, False)
    assert rel_err(f(y), y_ref) < 2e-2
    assert rel_err(f(dx), dx_ref) < 2e-2
    assert rel_err(f(dA), dA_ref[0]) < 2e-2
    assert rel_err(f(dB), dB_ref[0]) < 2e-2


@pytest.mark.parametrize("seed", range(12))
def test_chain3f_and_quad_kernel_random_shapes(seed):
    """Seeded random shapes for the long-T fp32 kernels (chain3f, the quad weight-gradient kernel where it applies): widths that
    are multiples of 4 but of nothing else, every rank count, ragged token counts, optional bias -- against the oracle."""
    import random
    from sow_amd import ops
    rnd = random.Random(1000 + seed)
    T = rnd.choice([8192, 8192 + 4 * rnd.randint(1, 300), 16384 + rnd.randint(1, 127)])
    d_in, d_out = 4 * rnd.randint(3, 160), 4 * rnd.randint(3, 160)
    r = rnd.choice([1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 63, 64])
    has_bias = rnd.random() < 0.5
    scale = rnd.choice([1.0, 0.5, 1.0 / r])
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(T, d_in, generator=gen, device=DEV)
    dy = torch.randn(T, d_out, generator=gen, device=DEV)
    A = torch.randn(d_in, r, generator=gen, device=DEV) * 0.05
    B = torch.randn(r, d_out, generator=gen, device=DEV) * 0.05
    bias = torch.randn(d_out, generator=gen, device=DEV) * 0.1 if has_bias else None
    y, h = ops.sow_forward(x, A, B, None, None, bias, scale)
    dx, dA, dB, db = ops.sow_backward(dy, x, h, A, B, None, None, scale, has_bias)
    cpu = lambda t: None if t is None else t.cpu()
    y_ref = O.sow_forward(x.cpu(), [A.cpu()], [B.cpu()], None, None, scale, cpu(bias))
    dx_ref, dA_ref, dB_ref, db_ref = O.sow_backward(dy.cpu(), x.cpu(), [A.cpu()], [B.cpu()], None, None, scale, has_bias)
    what = f"T={T} {d_in}->{d_out} r={r} bias={has_bias}"
    assert rel_err(y.cpu(), y_ref) < 1e-5, what
    assert rel_err(dx.cpu(), dx_ref) < 1e-5, what
    assert rel_err(dA.cpu(), dA_ref[0]) < 2e-5, what
    assert rel_err(dB.cpu(), dB_ref[0]) < 2e-5, what
    if has_bias:
        assert rel_err(db.cpu(), db_ref) < 2e-5, what


def test_fp32_long_t_forward_without_workspace_falls_back():
    """sow_forward_workspace_bytes is non-zero for fp32 inputs at T >= 8192 (factor planes of chain3f); a caller that passes
    NULL / 0 anyway still gets the right answer (the launch takes the kernel that needs no scratch)."""
    import ctypes
    from sow_amd import _lib, ops
    lib = _lib.load()
    T, d_in, d_out, r = 8192, 256, 192, 50
    assert lib.sow_forward_workspace_bytes(T, d_in, d_out, r, 0, _lib.ACC_NONE, _lib.F32) > 0
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(T, d_in, generator=gen, device=DEV)
    A = torch.randn(d_in, r, generator=gen, device=DEV) * 0.05
    B = torch.randn(r, d_out, generator=gen, device=DEV) * 0.05
    y = torch.empty(T, d_out, device=DEV)
    h = torch.empty(T * 64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.sow_forward(x.data_ptr(), A.data_ptr(), B.data_ptr(), None, None, None, y.data_ptr(), h.data_ptr(), T, d_in, d_out, r, 0,
                         _lib.ACC_NONE, ctypes.c_float(1.0), _lib.F32, None, 0, ctypes.c_void_p(stream))
    assert rc == 0
    y2, _ = ops.sow_forward(x, A, B, None, None, None, 1.0)
    y_ref = O.sow_forward(x.cpu(), [A.cpu()], [B.cpu()], None, None, 1.0, None)
    assert rel_err(y.cpu(), y_ref) < 1e-5 and rel_err(y2.cpu(), y_ref) < 1e-5
