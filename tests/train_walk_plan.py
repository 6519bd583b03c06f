"""The event walks of tests/test_gpu_train_walk.py (a plain module: importable without a GPU, no torch).

A walk is one model (the two-block Encoder of test_gpu_bias_bucket.py: six biased SoWLinear layers per block, q / k / v
siblings) and a list of events of a training loop.  Each event reaches a branch of the host-side state that lives between
calls: the sinks' `queued` / `pending` / workspace (sow_amd/dp.py), the bucket's block queues and the cached reduction
descriptors (FactorBucket._flush_block, ops.DeferredReduce), the parked sibling outputs (sow_amd/group.py), the routes of
SoWLinear.forward (grad, no-grad, skinny, SOW_FUSE_ACC), FactorAdamW's per-group steps and accumulate()'s rebinding.

`plan(seed)` returns the walks, deterministically: hand-written ones, one per named transition, then seeded ones of 10 to 14
events.  Token counts come from TS: the edges of the skinny route (32), of the 64-token tile, and of the streaming / grouped
threshold (8192); exactly one walk uses T_FUSE, where a low-rank accumulator takes SOW_FUSE_ACC, the persistent grids and the
row-owner plan.  `ref_cost(walk)` counts the multiply-adds of the float64 products the runner forms (as fuzz_plan.ref_cost
counts a case's); the CPU test keeps every walk under fuzz_plan.REF_COST_CAP.
"""
from __future__ import annotations

import dataclasses
import random
from typing import List, Tuple

SEED = 20261019
TS = (1, 31, 32, 33, 64, 65, 700, 8192, 8193, 8257)
T_FUSE = 32769
GEOMETRIES = ((96, 200), (128, 264))
DTYPES = ("bf16", "f16", "f32", "f32-autocast")     # f32-autocast: fp32 master factors under torch.autocast(bfloat16)
R_ACC = 24                                           # the low-rank accumulator Encoder builds (test_gpu_bias_bucket.R_ACC)
GRAD_KINDS = ("step", "micro", "ckpt_step", "partial_step", "tied_step")
KINDS = GRAD_KINDS + ("eval", "accumulate", "opt_step", "zero_grad", "reset_state", "regroup", "autocast")
REGROUP_MODES = ("ungrouped", "grouped", "shared")
DROPS = ("value", "query", "mlp")


@dataclasses.dataclass(frozen=True)
class Model:
    hidden: int
    inter: int
    dtype: str                  # one of DTYPES
    rank: int
    bias: bool                  # every layer of Encoder is biased
    acc: str                    # "none" | "dense" | "lowrank": the accumulator the model starts with
    bucket_biases: bool         # FactorBucket(factor_parameters(net, biases=...)): False leaves the biased layers on autograd
    grouping: str = "ungrouped"  # the sibling grouping the walk starts with (REGROUP_MODES)


@dataclasses.dataclass(frozen=True)
class Event:
    kind: str                   # one of KINDS
    T: int = 0                  # tokens of a forward (GRAD_KINDS, eval)
    eval_T: int = 0             # step: a no-grad forward of eval_T tokens between its forward and its backward (0: none)
    reentrant: bool = False     # ckpt_step: torch.utils.checkpoint(use_reentrant=...)
    drop: str = ""              # partial_step: "value" | "query" (that sibling of block 0 is not called: the grouped backward gets
                                # a None dY, and -- query being the sibling that is called first -- its output stays parked
                                # for the next forward to find) | "mlp" (block 1's intermediate + output do not run)
    group: int = 0              # reset_state: the param group (0 factors, 1 biases)
    mode: str = ""              # regroup: one of REGROUP_MODES
    on: bool = False            # autocast

    def __str__(self):
        extra = {"step": f"({self.T}" + (f", eval {self.eval_T})" if self.eval_T else ")"), "micro": f"({self.T})",
                 "eval": f"({self.T})", "ckpt_step": f"({self.T}, reentrant={self.reentrant})",
                 "partial_step": f"({self.T}, {self.drop})", "tied_step": f"({self.T})", "reset_state": f"({self.group})",
                 "regroup": f"({self.mode})", "autocast": f"({'on' if self.on else 'off'})"}
        return self.kind + extra.get(self.kind, "")


@dataclasses.dataclass(frozen=True)
class Walk:
    id: str
    model: Model
    events: Tuple[Event, ...]


def step(T, eval_T=0):
    return Event("step", T=T, eval_T=eval_T)


def micro(T):
    return Event("micro", T=T)


def ev(T):
    return Event("eval", T=T)


def ckpt(T, reentrant):
    return Event("ckpt_step", T=T, reentrant=reentrant)


def partial(T, drop):
    return Event("partial_step", T=T, drop=drop)


def tied(T):
    return Event("tied_step", T=T)


def regroup(mode):
    return Event("regroup", mode=mode)


ACC, OPT, ZERO = Event("accumulate"), Event("opt_step"), Event("zero_grad")


def reset(group):
    return Event("reset_state", group=group)


def autocast(on):
    return Event("autocast", on=on)


# ---- the transitions the plan has to hold (test_train_walk_plan_cpu.py) ------------------------------------------------------
def grad_events(walk: Walk) -> List[Event]:
    """The events of a walk without its zero_grad events: `a -> b` below means adjacent in this list."""
    return [e for e in walk.events if e.kind != "zero_grad"]


TRANSITIONS = {
    "step(T<=8192) -> step(T>8192)": lambda a, b: a.kind == b.kind == "step" and a.T <= 8192 < b.T,
    "step(T>8192) -> step(T<=8192)": lambda a, b: a.kind == b.kind == "step" and b.T <= 8192 < a.T,
    "step(T1) -> micro(T2 != T1)": lambda a, b: a.kind == "step" and b.kind == "micro" and a.T != b.T,
    "step -> step, same T": lambda a, b: a.kind == b.kind == "step" and a.T == b.T,
    "eval inside a step": lambda a, b: b.kind == "step" and b.eval_T > 0,
    "accumulate -> step": lambda a, b: a.kind == "accumulate" and b.kind == "step",
    "accumulate -> opt_step": lambda a, b: a.kind == "accumulate" and b.kind == "opt_step",
    "regroup -> step": lambda a, b: a.kind == "regroup" and b.kind == "step",
    "partial_step -> step": lambda a, b: a.kind == "partial_step" and b.kind == "step",
    "tied_step -> step": lambda a, b: a.kind == "tied_step" and b.kind == "step",
    "ckpt_step -> step": lambda a, b: a.kind == "ckpt_step" and b.kind == "step",
    "reset_state -> opt_step": lambda a, b: a.kind == "reset_state" and b.kind == "opt_step",
}


def transitions(walk: Walk) -> set:
    ge = grad_events(walk)
    return {name for a, b in zip(ge, ge[1:]) for name, f in TRANSITIONS.items() if f(a, b)}


# ---- float64 reference work ---------------------------------------------------------------------------------------------
def layer_shapes(m: Model):
    """(d_in, d_out) of the six layers of one block: query, key, value, dense, intermediate, output."""
    return [(m.hidden, m.hidden)] * 4 + [(m.hidden, m.inter), (m.inter, m.hidden)]


def acc_after(m: Model, n_accumulate: int):
    """(kind, r_acc) of every layer after n accumulate() calls: the first call re-factors the accumulator by a truncated QR
    of rank min(rank, widths), every further one grows it by `rank` (SoWLinear.accumulate, virtual_rank)."""
    if n_accumulate == 0:
        return m.acc, (R_ACC if m.acc == "lowrank" else 0)
    return "lowrank", min(m.rank * n_accumulate, m.hidden)


def ref_cost(walk: Walk) -> float:
    """Multiply-adds of the float64 products of the runner's checks, counted as if every backward pass had its weight
    gradients and every no-grad pass its output held to float64 (an upper bound: the runner compares bit for bit with the
    autograd copy wherever both cut the token axis alike):
      a backward pass   h, dh, dA and its squares, dB and its squares          3 T (d_in + d_out) r
                        + the shared-input dX of q / k / v (dh A^T and squares) 2 T d_in r per sibling
      a no-grad pass    x A, h B and squares                                    T (d_in + 2 d_out) r
                        + dense: x W and squares                                2 T d_in d_out
                        + low-rank: x Q, (x Q) R and their squares              2 T (d_in + d_out) r_acc
    A step with an eval inside runs twice (with and without the eval)."""
    m, n_acc, cost = walk.model, 0, 0.0
    shapes = layer_shapes(m)
    for e in walk.events:
        if e.kind == "accumulate":
            n_acc += 1
        kind, r_acc = acc_after(m, n_acc)
        if e.kind in GRAD_KINDS:
            one = sum(3.0 * e.T * (i + o) * m.rank for i, o in shapes) + 3 * 2.0 * e.T * m.hidden * m.rank
            cost += 2 * one * (2 if e.eval_T else 1)
        for T in ([e.T] if e.kind == "eval" else [e.eval_T] if e.eval_T else []):
            for i, o in shapes:
                c = 1.0 * T * (i + 2 * o) * m.rank
                c += 2.0 * T * i * o if kind == "dense" else 2.0 * T * (i + o) * r_acc if kind == "lowrank" else 0.0
                cost += 2 * c
    return cost


# ---- the walks -------------------------------------------------------------------------------------------------------------
def _hand() -> List[Walk]:
    small, big = GEOMETRIES
    M = Model
    return [
        # T up then down across 8192 with the bucket attached: the reduction descriptors of a block depend on T; two equal
        # steps first (the cached descriptors are reused), then the row-owner plan, then back
        Walk("T_up_down_bf16", M(*big, "bf16", 8, True, "none", True, "grouped"),
             (step(700), ZERO, step(700), ZERO, step(8257), ZERO, step(8192), ZERO, step(8193), ZERO, step(64), OPT)),
        # gradient accumulation with micro-batches of other sizes: every sink is `pending` when the second backward arrives
        Walk("micro_other_T_f16", M(*small, "f16", 8, True, "dense", True),
             (step(700), micro(8257), ZERO, step(8193), micro(65), micro(65), OPT, ZERO, step(65))),
        # a no-grad forward between a step's forward and its backward, on both sides of the skinny route; eval on its own
        Walk("eval_inside_step_bf16", M(*small, "bf16", 8, True, "dense", True, "grouped"),
             (step(700, eval_T=31), ZERO, ev(32), ev(33), step(8193, eval_T=65), ZERO, ev(1), step(64, eval_T=8257), ev(700))),
        # activation checkpointing in both modes: the first forward takes the no-grad route (reentrant) and the backward
        # re-runs the block
        Walk("checkpoint_f32", M(*small, "f32", 8, True, "none", True, "grouped"),
             (ckpt(700, True), step(700), ZERO, ckpt(8193, False), ZERO, step(8193), ZERO, ckpt(31, True), ZERO, ckpt(65, False),
              step(65))),
        # a sibling without a gradient (grouped: a None dY) and a block whose MLP did not run: incomplete blocks wait for finalize()
        Walk("partial_bf16", M(*big, "bf16", 16, True, "none", True, "grouped"),
             (partial(700, "value"), step(700), ZERO, partial(700, "query"), step(700), ZERO, partial(8257, "mlp"), step(8257), ZERO,
              regroup("ungrouped"), partial(65, "value"), step(65), OPT)),
        # one layer called twice in a forward: its sink is `queued`, then `pending`, when the second backward pass arrives
        Walk("tied_f16", M(*small, "f16", 8, True, "none", True),
             (tied(700), step(700), ZERO, tied(8193), ZERO, step(8193), ZERO, regroup("grouped"), tied(33), step(33))),
        # accumulate() with the bucket attached, from no accumulator and from an existing one: rebinding, new kernels, new
        # workspaces and descriptors for every layer
        Walk("accumulate_bf16", M(*small, "bf16", 8, True, "none", True, "grouped"),
             (step(700), OPT, ZERO, ACC, step(700), OPT, ZERO, step(700), ACC, OPT, ZERO, step(8193), reset(0), OPT)),
        # regrouping between steps: ungrouped, grouped and shared-input siblings on the same bucket
        Walk("regroup_bf16", M(*big, "bf16", 8, True, "none", True),
             (step(8257), ZERO, regroup("grouped"), step(8257), ZERO, regroup("shared"), step(8257), ZERO, step(700), ZERO,
              regroup("ungrouped"), step(8257), OPT)),
        # fp32 master factors in and out of autocast: the run dtype of the bucket's blocks changes between steps
        Walk("autocast_toggle_f32", M(*big, "f32", 8, True, "dense", True, "grouped"),
             (step(700), ZERO, autocast(True), step(700), ZERO, step(8257), ZERO, autocast(False), step(8257), ZERO, autocast(True),
              ev(33), step(65), OPT)),
        # the one long walk: SOW_FUSE_ACC, the persistent grids and the row-owner plan of a low-rank-accumulator block
        Walk("fuse_acc_T32769_bf16", M(*big, "bf16", 8, True, "lowrank", True, "grouped"),
             (step(T_FUSE, eval_T=33), ZERO, step(700), micro(T_FUSE), OPT)),
    ]


def _seeded(g: random.Random, n: int) -> List[Walk]:
    out = []
    dts = ["bf16", "f16", "f32", "f32-autocast", "bf16", "f16", "f32-autocast", "bf16"]
    for w in range(n):
        dt = dts[w % len(dts)]
        geo = GEOMETRIES[g.randrange(2)]
        acc = g.choice(["none", "dense", "lowrank"])
        m = Model(*geo, dt, g.choice([8, 8, 16]), True, acc, w != 3, g.choice(REGROUP_MODES))
        n_ev = g.randint(10, 14)
        evs: List[Event] = [step(g.choice(TS))]
        n_acc = 0
        while len(evs) < n_ev:
            prev = evs[-1]
            kinds = ["step"] * 4 + ["zero_grad"] * 3 + ["opt_step"] * 2 + ["eval", "ckpt_step", "partial_step", "tied_step",
                                                                          "regroup", "reset_state"]
            if prev.kind in ("step", "micro") and not prev.eval_T:
                kinds += ["micro"] * 2
            if n_acc < 1:
                kinds.append("accumulate")
            if dt == "f32":
                kinds.append("autocast")
            k = g.choice(kinds)
            T = g.choice(TS)
            if k == "step":
                e = step(T, eval_T=g.choice(TS) if g.random() < 0.25 else 0)
            elif k == "micro":
                e = micro(T)
            elif k == "eval":
                e = ev(T)
            elif k == "ckpt_step":
                e = ckpt(T, g.random() < 0.5)
            elif k == "partial_step":
                e = partial(T, g.choice(DROPS))
            elif k == "tied_step":
                e = tied(T)
            elif k == "regroup":
                e = regroup(g.choice(REGROUP_MODES))
            elif k == "reset_state":
                e = reset(g.randrange(2) if m.bucket_biases else 0)
            elif k == "autocast":
                e = autocast(not next((x.on for x in reversed(evs) if x.kind == "autocast"), False))
            elif k == "accumulate":
                e, n_acc = ACC, n_acc + 1
            else:
                e = OPT if k == "opt_step" else ZERO
            if e.kind == prev.kind and e.kind in ("zero_grad", "regroup", "reset_state", "autocast", "accumulate"):
                continue
            evs.append(e)
        tag = f"seeded{w}_{dt}_{geo[0]}x{geo[1]}_r{m.rank}_{acc}" + ("" if m.bucket_biases else "_nobias")
        out.append(Walk(tag, m, tuple(evs)))
    return out


def plan(seed: int = SEED) -> List[Walk]:
    return _hand() + _seeded(random.Random(seed), 8)
