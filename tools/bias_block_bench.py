#!/usr/bin/env python3
"""Biased layers in the flat bucket: one roberta-base encoder block on the block-level path against autograd.

The block: the six biased SoWLinear layers of a roberta-base encoder layer (query, key, value, attention.output.dense:
768 -> 768; intermediate.dense: 768 -> 3072; output.dense: 3072 -> 768), rank 8, a dense accumulator (what
decompose="keep" leaves), query / key / value grouped (group_siblings).  Timed through the module surface, Python
included, HIP events around forward + backward + FactorBucket.finalize():
  attached  FactorBucket(factor_parameters(block, biases=True)).attach(block): every layer runs its data gradient as it
            arrives, ONE weight-gradient launch covers the block, dbias comes out of the same partial sums;
  autograd  FactorBucket(factor_parameters(block)): the biased layers are not attached (the behaviour before biases could
            be bucket members): per-layer backward calls, per-parameter AccumulateGrad.
The two variants alternate call by call in one process; WARM warm-up steps, then REPEATS windows of TIMED steps each: the
figure of a variant is the median of the window medians, its spread the distance between the largest and the smallest
window median.  Every step takes the next copy of the input, rotating over more than 256 MiB.
Also timed: FactorAdamW.step() on the attached bucket with two param groups (sow_adamw_flat_seg) against one group
(sow_adamw_flat).

  python tools/bias_block_bench.py [--out profiles/bias_bucket.txt]
  python tools/bias_block_bench.py --one T bf16|autocast attached|autograd        (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import copy
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import FactorBucket, SoWLinear, _lib, factor_parameters, group_siblings  # noqa: E402
from sow_amd.optimizer import FactorAdamW  # noqa: E402

DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
HIDDEN, INTER, RANK = 768, 3072, 8
WARM, TIMED, REPEATS = 10, 48, 5
VARIANTS = ("attached", "autograd")


class Attention(nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.query, self.key, self.value, self.dense = (mk(HIDDEN, HIDDEN) for _ in range(4))


class Block(nn.Module):
    """The six SoW layers of an encoder layer with element-wise glue in place of the attention product and the norms."""

    def __init__(self, mk):
        super().__init__()
        self.attention = Attention(mk)
        self.intermediate, self.output = mk(HIDDEN, INTER), mk(INTER, HIDDEN)

    def forward(self, x):
        a = self.attention
        q, k, v = a.query(x), a.key(x), a.value(x)
        x = x + a.dense(torch.tanh(q) * torch.sigmoid(k) + v)
        return x + self.output(torch.tanh(self.intermediate(x)))


class Model(nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.layer = nn.ModuleList([Block(mk)])     # names `layer.0.attention.query` ...: one block for FactorBucket

    def forward(self, x):
        return self.layer[0](x)


def make_block(dtype):
    g = torch.Generator().manual_seed(1)

    def mk(i, o):
        m = SoWLinear(i, o, bias=True, rank=RANK, scale=1.0, init_method="normal", device=DEV, dtype=dtype)
        rnd = lambda *s, std: (torch.randn(*s, generator=g) * std).to(DEV, dtype)   # noqa: E731
        m.downscale_weights[0].data.copy_(rnd(i, RANK, std=0.05))
        m.upscale_weights[0].data.copy_(rnd(RANK, o, std=0.05))
        m.bias.data.copy_(rnd(o, std=0.1))
        m.acc_downweight = nn.Parameter(rnd(i, o, std=0.02), requires_grad=False)
        return m

    return Model(mk)


class Setup:
    def __init__(self, T, mode):
        self.T, self.autocast = T, mode == "autocast"
        pdt = F32 if self.autocast else BF16
        base = make_block(pdt)
        per_copy = T * HIDDEN * (4 if self.autocast else 2)
        self.copies = max(2, -(-288 * 1024 * 1024 // per_copy))
        g = torch.Generator(device="cuda").manual_seed(2)
        self.x = [torch.randn(T, HIDDEN, device=DEV, generator=g).to(pdt).requires_grad_(True) for _ in range(self.copies)]
        self.w = torch.randn(T, HIDDEN, device=DEV, generator=g).to(pdt)      # the block's output has the input's dtype
        self.model, self.bucket = {}, {}
        for v in VARIANTS:
            m = copy.deepcopy(base)
            group_siblings(m)
            b = FactorBucket(factor_parameters(m, biases=(v == "attached")))
            n = b.attach(m)
            assert n == (6 if v == "attached" else 0), (v, n)
            self.model[v], self.bucket[v] = m, b

    def step(self, v, j):
        x = self.x[j % self.copies]
        x.grad = None
        with torch.autocast("cuda", dtype=BF16, enabled=self.autocast):
            y = self.model[v](x)
        y.backward(self.w)
        self.bucket[v].finalize()
        return y, x.grad


def measure(S):
    for j in range(WARM):
        for v in VARIANTS:
            S.bucket[v].zero_grad()
            S.step(v, j)
    torch.cuda.synchronize()
    meds = {v: [] for v in VARIANTS}
    j = 0
    for _ in range(REPEATS):
        times = {v: [] for v in VARIANTS}
        for _ in range(TIMED):
            for v in VARIANTS:
                S.bucket[v].zero_grad()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                S.step(v, j)
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1e3)
            j += 1
        for v in VARIANTS:
            meds[v].append(statistics.median(times[v]))
    return {v: (statistics.median(m), max(m) - min(m)) for v, m in meds.items()}


def same_results(S):
    """Faster and different is not faster: y and dX bit for bit, the gradients to max |difference| / max |value|."""
    out, grads = {}, {}
    for v in VARIANTS:
        S.bucket[v].zero_grad()
        y, dx = S.step(v, 0)
        torch.cuda.synchronize()
        out[v] = (y.detach().clone(), dx.detach().clone())
        grads[v] = [p.grad.detach().float().clone() for p in factor_parameters(S.model[v], biases=True)]
    same = torch.equal(out["attached"][0], out["autograd"][0]) and torch.equal(out["attached"][1], out["autograd"][1])
    n_fac = len(factor_parameters(S.model["attached"]))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))   # noqa: E731
    d_fac = max(rel(a, b) for a, b in zip(grads["attached"][:n_fac], grads["autograd"][:n_fac]))
    d_bias = max(rel(a, b) for a, b in zip(grads["attached"][n_fac:], grads["autograd"][n_fac:]))
    return same, d_fac, d_bias


def measure_optimizer(S):
    """FactorAdamW.step() on the attached bucket: two param groups against one."""
    b = S.bucket["attached"]
    n_fac = len(factor_parameters(S.model["attached"]))
    opts = {"two groups": FactorAdamW(b, param_groups=[{"params": b.params[:n_fac], "lr": 1e-3, "weight_decay": 0.1},
                                                       {"params": b.params[n_fac:], "lr": 1e-4, "weight_decay": 0.0}]),
            "one group": FactorAdamW(b, lr=1e-3, weight_decay=0.1)}
    for o in opts.values():
        for _ in range(WARM):
            o.step()
    torch.cuda.synchronize()
    meds = {k: [] for k in opts}
    for _ in range(REPEATS):
        times = {k: [] for k in opts}
        for _ in range(4 * TIMED):
            for k, o in opts.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                o.step()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        for k in opts:
            meds[k].append(statistics.median(times[k]))
    return {k: (statistics.median(m), max(m) - min(m)) for k, m in meds.items()}, b.padded_numel


def sweep(out_path):
    lines = [f"# tools/bias_block_bench.py on {torch.cuda.get_device_name(0)}; sow_version {_lib.load().sow_version()}",
             "# one roberta-base encoder block: 6 biased SoWLinear layers (768 / 3072), rank 8, dense accumulator, q / k / v grouped",
             f"# us per forward + backward + finalize() through the module surface (Python included): median of {REPEATS} window "
             f"medians ({TIMED} steps each, {WARM} warm-up), +- = spread of the window medians; the input rotates over > 256 MiB",
             "# attached = biases in the bucket, block-level weight gradients; autograd = biases outside, layers not attached",
             "# y/dX = bit-identical between the variants; dfac / dbias = max |attached - autograd| / max |autograd| over the gradients",
             f"{'T':>6} {'dtype':>9} | {'attached':>16} {'autograd':>16} {'att/auto':>8} | {'y/dX':>5} {'dfac':>7} {'dbias':>7}"]
    print("\n".join(lines), flush=True)
    cell = lambda v: f"{v[0]:10.1f}+-{v[1]:<4.1f}"   # noqa: E731
    last = None
    for T in (4096, 16384):
        for mode in ("bf16", "autocast"):
            S = Setup(T, mode)
            same, d_fac, d_bias = same_results(S)
            m = measure(S)
            line = (f"{T:6d} {mode:>9} | {cell(m['attached'])} {cell(m['autograd'])} {m['attached'][0] / m['autograd'][0]:8.3f} | "
                    f"{'same' if same else 'DIFF':>5} {d_fac:7.1e} {d_bias:7.1e}")
            print(line, flush=True)
            lines.append(line)
            if mode == "bf16":
                last = S
            else:
                del S
            torch.cuda.empty_cache()
    o, n = measure_optimizer(last)
    line = (f"# FactorAdamW.step() on the attached bf16 bucket ({n} elements): two param groups (sow_adamw_flat_seg) "
            f"{cell(o['two groups']).strip()} us, one group (sow_adamw_flat) {cell(o['one group']).strip()} us")
    print(line, flush=True)
    lines.append(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def one(T, mode, variant):
    S = Setup(T, mode)
    for j in range(20):
        S.bucket[variant].zero_grad()
        S.step(variant, j)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, metavar=("T", "MODE", "VARIANT"))
    a = ap.parse_args()
    if a.one:
        one(int(a.one[0]), a.one[1], a.one[2])
    else:
        sweep(a.out)
