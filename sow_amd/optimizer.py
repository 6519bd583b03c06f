"""TT optimizers -- host-side mirror of tn_gradient/optimizer/ttadam.py and ttsgd.py.

Optimizer state is held as TensorTrain cores between steps (decompress -> dense update -> recompress);
the dense update is one fused kernel (sow_ttadam_dense), (de)compression uses the QR / GEMM kernels.
FactorAdamW is the fused flat-bucket AdamW for the SoW factor group.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, Tuple

import torch
import torch.nn as nn

from . import ops
from .tt import TensorTrain


class TTAdam(torch.optim.Optimizer):
    """ttadam.py:10-117."""

    def __init__(self, params: Iterable[nn.parameter.Parameter], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0, amsgrad: bool = False, correct_bias: bool = True):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, correct_bias=correct_bias)
        super().__init__(params, defaults)

    batched = True    # TT groups step through sow_ttadam_batch (one launch sequence for all parameters); False: per parameter

    def _step_tt_group_batched(self, group) -> set:
        """ttadam.py:68-115 for every parameter of a TT group in ONE C call (sow_ttadam_batch): reconstruct m and v, clamp,
        Adam update, re-decompose -- 1 + 4 (order - 1) launches per 8 parameters instead of ~40 per parameter.  Returns the
        ids of the parameters it stepped; the others (non-fp32, CPU, ranks the kernels do not cover) keep the loop below."""
        import ctypes

        from . import _lib
        from .tt import _empty_train, _tt_desc
        lib = _lib.load()
        ranks = list(group["ranks"])
        beta1, beta2 = group["betas"]
        items, keep, done = [], [], set()
        for p in group["params"]:
            if p.grad is None or p.grad.is_sparse or p.dim() != 2:
                continue
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                continue
            grad = p.grad if (p.grad.dtype == torch.float32 and p.grad.stride(1) == 1) else p.grad.float().contiguous()
            state = self.state[p]
            has = "exp_avg" in state and "exp_avg_sq" in state
            if has:
                tm, tv = state["exp_avg"], state["exp_avg_sq"]
                if not (isinstance(tm, TensorTrain) and isinstance(tv, TensorTrain) and list(tm.ranks) == ranks
                        and list(tv.ranks) == ranks):
                    continue
            else:
                tm, tv = _empty_train(ranks, p.shape, p.device), _empty_train(ranks, p.shape, p.device)
            dm = _tt_desc(tm.cores, tm.ranks, tm.input_shape, tm.output_shape, p.shape[0], p.shape[1])
            dv = _tt_desc(tv.cores, tv.ranks, tv.input_shape, tv.output_shape, p.shape[0], p.shape[1])
            if dm is None or dv is None:
                continue
            step = state.get("step", 0) + 1
            step_size = group["lr"]
            if group["correct_bias"]:
                step_size = step_size * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
            nws = int(lib.sow_ttadam_workspace_bytes(ctypes.byref(dm)))
            ws = torch.empty(nws, dtype=torch.uint8, device=p.device)
            it = _lib.TtAdamItem()
            it.m, it.v = dm, dv
            it.param, it.grad, it.ld_param, it.ld_grad = p.data_ptr(), grad.data_ptr(), p.stride(0), grad.stride(0)
            it.step_size = step_size
            it.lr_times_wd = group["lr"] * group["weight_decay"] if group["weight_decay"] > 0.0 else 0.0
            it.has_state, it.workspace, it.workspace_bytes = int(has), ws.data_ptr(), nws
            items.append(it)
            keep.append((p, grad, ws, tm, tv, step))
        if not items:
            return done
        by_dev = {}
        for it, k in zip(items, keep):
            by_dev.setdefault(k[0].device, []).append((it, k))
        for dev, lst in by_dev.items():
            arr = (_lib.TtAdamItem * len(lst))(*[it for it, _ in lst])
            ops._launch(dev, "sow_ttadam_batch", lib.sow_ttadam_batch, arr, len(lst), beta1, beta2, group["eps"])
            for _, (p, _, _, tm, tv, step) in lst:
                st = self.state[p]
                st["step"], st["exp_avg"], st["exp_avg_sq"] = step, tm, tv
                done.add(id(p))
        return done

    @torch.no_grad()
    def step(self, closure: Callable = None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            done = self._step_tt_group_batched(group) if ("ranks" in group and self.batched) else set()
            for p in group["params"]:
                if p.grad is None or id(p) in done:
                    continue
                grad = p.grad
                if grad.is_sparse:
                    raise RuntimeError("TTAdam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if "step" not in state:
                    state["step"] = 0
                tt_mode = "ranks" in group
                clamp = False
                if "exp_avg" not in state:
                    m = torch.zeros_like(grad, dtype=torch.float32)
                elif tt_mode:
                    m = state["exp_avg"].to_matrix(grad.shape).contiguous().float()   # ttadam.py:71-74
                else:
                    m = state["exp_avg"]
                if "exp_avg_sq" not in state:
                    v = torch.zeros_like(grad, dtype=torch.float32)
                elif tt_mode:
                    v = state["exp_avg_sq"].to_matrix(grad.shape).contiguous().float()  # ttadam.py:79-84
                    clamp = True                                                         # v[v < 0] = 0
                else:
                    v = state["exp_avg_sq"]
                state["step"] += 1
                beta1, beta2 = group["betas"]
                step_size = group["lr"]
                if group["correct_bias"]:
                    step_size = step_size * math.sqrt(1.0 - beta2 ** state["step"]) / (1.0 - beta1 ** state["step"])
                lr_wd = group["lr"] * group["weight_decay"] if group["weight_decay"] > 0.0 else 0.0
                if p.dtype == torch.float32 and p.is_contiguous():
                    ops.ttadam_dense_(p.data, grad.contiguous().float(), m, v, beta1=beta1, beta2=beta2, eps=group["eps"],
                                      step_size=step_size, lr_times_wd=lr_wd, clamp_v=clamp)
                else:
                    p32 = p.data.float().contiguous()
                    ops.ttadam_dense_(p32, grad.contiguous().float(), m, v, beta1=beta1, beta2=beta2, eps=group["eps"],
                                      step_size=step_size, lr_times_wd=lr_wd, clamp_v=clamp)
                    p.data.copy_(p32)
                if tt_mode:
                    state["exp_avg"] = TensorTrain.from_matrix(m, ranks=group["ranks"], padding=True)     # ttadam.py:113-115
                    state["exp_avg_sq"] = TensorTrain.from_matrix(v, ranks=group["ranks"], padding=True)
                else:
                    state["exp_avg"], state["exp_avg_sq"] = m, v
        return loss


class TTRAdam(torch.optim.Optimizer):
    """Empty stub in the reference as well (ttadam.py:120-121)."""
    pass


class TTSGD(torch.optim.Optimizer):
    """ttsgd.py:8-86, including its quirk: the momentum buffer stored at the first step is never
    updated afterwards (the new value is bound to a local name only, ttsgd.py:68-69)."""

    def __init__(self, params: Iterable[nn.parameter.Parameter], lr: float = 1e-3, momentum: float = 0.9, dampening: float = 0,
                 weight_decay: float = 0, nesterov: bool = False):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)

    @torch.no_grad()
    def step(self, closure: Callable = None):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                grad_shape = grad.shape
                if grad.is_sparse:
                    raise RuntimeError("TTSGD does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if "step" not in state:
                    state["step"] = 0
                tt_mode = "ranks" in group
                d_p = TensorTrain.from_matrix(grad, ranks=group["ranks"], padding=True) if tt_mode else grad
                if group["weight_decay"] != 0:
                    d_p = d_p.add(p, alpha=group["weight_decay"])  # TensorTrain has no .add: raises like ttsgd.py:62
                if group["momentum"] != 0:
                    if "momentum_buffer" not in state:
                        buf = state["momentum_buffer"] = d_p.clone().detach()
                    else:
                        buf = state["momentum_buffer"]
                        buf = group["momentum"] * buf + (1 - group["dampening"]) * d_p
                    d_p = d_p + group["momentum"] * buf if group["nesterov"] else buf
                if tt_mode:
                    d_p = d_p.to_matrix(grad_shape)
                d_p = d_p.to(p.dtype).contiguous()
                if p.is_contiguous():
                    ops.axpby_(d_p, p.data, -group["lr"], 1.0)   # p += -lr * d_p   (ttsgd.py:78)
                else:
                    tmp = p.data.contiguous()
                    ops.axpby_(d_p, tmp, -group["lr"], 1.0)
                    p.data.copy_(tmp)
                if group["weight_decay"] > 0.0:
                    ops.axpby_(p.data.clone(), p.data, -group["lr"] * group["weight_decay"], 1.0)
        return loss


class FactorAdamW:
    """Fused AdamW for the SoW factor parameter group (simple_train.py:502-506): all factors and
    their gradients live in ONE flat buffer each, so the step is one kernel launch and the DP
    all-reduce one collective (see sow_amd/dp.py).  torch.optim.AdamW semantics.

    param_groups: a list of torch-style dicts {"params": [...], "lr": ..., "weight_decay": ...} that together hold every
    parameter of the bucket exactly once (ValueError otherwise) -- the factors at sow_lr with weight decay and the biases
    at lr without, run_glue.py:796-808.  betas and eps are shared; a group without "lr" / "weight_decay" takes the
    constructor's.  Each group has its own step count, reset_state(group_id) resets one group, and step() is still ONE
    launch (sow_adamw_flat_seg over the groups' segments of the flat buffer).  Without param_groups the object is the
    one-group optimizer it has always been (sow_adamw_flat, the same state_dict keys).

    Clipping and skipping without a host read: step(max_grad_norm=..., loss_scale=..., found_inf=..., skip_nonfinite=...)
    takes the global norm of the flat gradient on the device (FactorBucket.grad_stats) and makes ONE
    sow_adamw_flat_seg_stats launch that reads its gradient multiplier and its go / no-go flag from that record: the
    gradient is neither rewritten nor rounded a second time, and the step can be captured in a HIP graph.  With
    skip_nonfinite the optimizer owns one device int32 counter per param group (plus one for the whole optimizer when it
    has groups) that counts the skipped steps; the host step counts advance as always and the kernel corrects the bias
    for step - counter.  state_dict() reads the counters (the one host read), folds them into the step counts and zeroes
    them, so a checkpoint holds true step counts under today's keys."""

    # class-level defaults (an instance sets them when it first needs them)
    last_grad_stats = None     # the GradStats of the last step() that took the device-record path
    _armed_stats = None        # sow_amd.clip_grad_norm_: consumed by the next step()
    _stats_out = None
    _counters = None           # device int32 skip counters, created by the first skip_nonfinite use

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, state_dtype=None, param_groups=None):
        self.bucket = bucket
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        sd = state_dtype or bucket.flat_param.dtype
        self.exp_avg = torch.zeros_like(bucket.flat_param, dtype=sd)
        self.exp_avg_sq = torch.zeros_like(bucket.flat_param, dtype=sd)
        self.step_count = 0
        self._groups = None
        if param_groups is not None:
            slot = {id(p): i for i, p in enumerate(bucket.params)}
            owner = [None] * len(bucket.params)
            self._groups = []
            for gi, g in enumerate(param_groups):
                g = dict(g)
                g["params"] = list(g["params"])
                g.setdefault("lr", lr)
                g.setdefault("weight_decay", weight_decay)
                g["betas"], g["eps"] = betas, eps
                for p in g["params"]:
                    i = slot.get(id(p))
                    if i is None:
                        raise ValueError(f"FactorAdamW: a parameter of param group {gi} is not in the bucket")
                    if owner[i] is not None:
                        raise ValueError(f"FactorAdamW: bucket parameter {i} is in param groups {owner[i]} and {gi}")
                    owner[i] = gi
                self._groups.append(g)
            missing = [i for i, o in enumerate(owner) if o is None]
            if missing:
                raise ValueError(f"FactorAdamW: {len(missing)} bucket parameters are in no param group (first: slot {missing[0]})")
            self._owner = owner
            self.group_steps = [0] * len(self._groups)

    def _sync_from_group(self):
        """Hyper-parameters written through param_groups[0] (what LR schedulers and drivers do: `group["lr"] = v`,
        simple_train.py:537-563) are the ones the next step() uses and state_dict() saves."""
        g = self.__dict__.get("_group")
        if g is not None:
            self.lr, self.betas, self.eps, self.weight_decay = g["lr"], g["betas"], g["eps"], g["weight_decay"]

    def _group_ranges(self):
        """[(group id, begin, end)] over the flat buffer, sorted: adjacent slots of one group merged, the 64-element
        padding of a slot belonging to the slot before it."""
        offs = list(self.bucket.offsets) + [self.bucket.padded_numel]
        out = []
        for i, gi in enumerate(self._owner):
            if out and out[-1][0] == gi:
                out[-1][2] = offs[i + 1]
            else:
                out.append([gi, offs[i], offs[i + 1]])
        return [tuple(r) for r in out]

    def segments(self, advance: int = 1):
        """The segment table the next step() launches: (begin, end, lr, weight_decay, step) per segment, each group's
        current hyper-parameters and its step count + `advance`.  A pure function of the bucket layout and the groups."""
        if self._groups is None:
            raise RuntimeError("FactorAdamW.segments: the optimizer was built without param_groups")
        return [(b, e, float(self._groups[gi]["lr"]), float(self._groups[gi]["weight_decay"]), self.group_steps[gi] + advance)
                for gi, b, e in self._group_ranges()]

    @property
    def skip_counters(self) -> torch.Tensor:
        """The device int32 skip counters (created zeroed on first use): entry g counts the skipped steps of param group g
        since its last reset; a grouped optimizer has one more, for step_count."""
        if self._counters is None:
            n = 1 if self._groups is None else len(self._groups) + 1
            self._counters = torch.zeros(n, dtype=torch.int32, device=self.bucket.flat_param.device)
        return self._counters

    def _fold_counters(self) -> None:
        """Read the skip counters (synchronises), take them off the host step counts and zero them."""
        if self._counters is None:
            return
        c = [int(x) for x in self._counters.tolist()]
        if any(c):
            if self._groups is None:
                self.step_count = max(0, self.step_count - c[0])
            else:
                self.group_steps = [max(0, s - k) for s, k in zip(self.group_steps, c)]
                self.step_count = max(0, self.step_count - c[-1])
            self._counters.zero_()

    def arm_grad_stats(self, stats) -> None:
        """Hand the next step() a record computed beforehand (sow_amd.clip_grad_norm_ does): that step() multiplies the
        gradient by stats.grad_mult, whatever its own keywords say, and the one after it is an ordinary step again."""
        self._armed_stats = stats

    def _check_layout(self):
        for p, o in zip(self.bucket.params, self.bucket.offsets):
            if p.data_ptr() != self.bucket.flat_param.data_ptr() + o * self.bucket.flat_param.element_size():
                raise RuntimeError("FactorAdamW.step: a factor no longer lives in the flat buffer (SoWLinear.accumulate() "
                                   "rebinds .data) -- call bucket.rebind() after accumulate(); sow_amd.accumulate(model) does")

    def step(self, grad_scale: float = 1.0, *, max_grad_norm=None, extra_sq_norm=None, loss_scale=None, found_inf=None,
             skip_nonfinite: bool = False, stats=None):
        """One AdamW step of the whole bucket.  grad_scale: a host multiplier of the gradient (1 / world size after a sum
        all-reduce).  With every keyword at its default (and nothing armed by clip_grad_norm_) this is the plain
        sow_adamw_flat / sow_adamw_flat_seg launch and returns None.  Otherwise -- max_grad_norm: clip the global norm
        (torch.nn.utils.clip_grad_norm_'s formula); extra_sq_norm: squared norm of gradients outside the bucket that count
        towards it; loss_scale: divide the gradient by it (float or 1-element float32 device tensor); found_inf: a device
        flag that marks the gradients as overflowed; skip_nonfinite: leave parameters and moments untouched when the norm is
        not finite or found_inf is set; stats: a GradStats computed beforehand instead of computing one here (the record
        holds its own scale, clipping and flag: giving max_grad_norm, extra_sq_norm, loss_scale, found_inf or another
        grad_scale along with it, or with a record armed by clip_grad_norm_, raises).  Returns the GradStats, also kept as
        last_grad_stats; nothing on this path reads device memory from the host.  Once skip_nonfinite has been used the
        skip counters exist, and from then on every step() -- a plain one included -- takes this path and reads them, so
        that the bias correction stays that of the effective step whatever form of step() follows a skipped one."""
        armed, self._armed_stats = self._armed_stats, None
        formed_here = {k: v for k, v in (("max_grad_norm", max_grad_norm), ("extra_sq_norm", extra_sq_norm),
                                         ("loss_scale", loss_scale), ("found_inf", found_inf)) if v is not None}
        if armed is None and stats is None and not formed_here and not skip_nonfinite and self._counters is None:
            return self._step_plain(grad_scale)
        if armed is not None:
            if stats is not None and stats is not armed:
                raise ValueError("FactorAdamW.step: stats= given while clip_grad_norm_ has armed another record")
            stats = armed
        if stats is not None:
            # the record already holds its scale, its clipping and its flag: a keyword that says otherwise would be ignored
            if float(grad_scale) not in (1.0, stats.grad_scale):
                raise ValueError(f"FactorAdamW.step: grad_scale={grad_scale} but the record of this step was formed with "
                                 f"{stats.grad_scale} -- pass the scale where the record is computed (clip_grad_norm_, "
                                 "grad_stats) only")
            if formed_here:
                raise ValueError(f"FactorAdamW.step: {', '.join(formed_here)} given together with a record computed beforehand "
                                 "-- pass them where the record is computed (clip_grad_norm_, grad_stats)")
        from . import ops
        ops._need_gpu(self.bucket.flat_param, self.bucket.flat_grad)
        self._sync_from_group()
        self.bucket.finalize()
        self._check_layout()
        if stats is None:
            if self._stats_out is None:
                self._stats_out = ops.GradStats(torch.empty(ops.GradStats.NBYTES, dtype=torch.uint8,
                                                            device=self.bucket.flat_grad.device))
            stats = self.bucket.grad_stats(grad_scale=grad_scale, max_norm=max_grad_norm, extra_sq_norm=extra_sq_norm,
                                           loss_scale=loss_scale, found_inf=found_inf,
                                           skip_counters=self.skip_counters if skip_nonfinite else None, out=self._stats_out)
        elif skip_nonfinite and stats.counters is not self.skip_counters:
            self.skip_counters.add_(stats.nonfinite)     # a record formed elsewhere: its flag is counted here, on the stream
        # Once the counters exist every step reads them, whatever its keywords: the host step counts still hold the
        # skipped steps until state_dict() folds them, and only the kernel can take them off without a host read.
        counted = self._counters is not None
        if self._groups is not None:
            segs = self.segments()
            cnt = [gi if counted else -1 for gi, _, _ in self._group_ranges()]
            self.group_steps = [s + 1 for s in self.group_steps]
            self.step_count += 1
        else:
            self.step_count += 1
            segs = [(0, self.bucket.padded_numel, float(self.lr), float(self.weight_decay), self.step_count)]
            cnt = [0 if counted else -1]
        ops.adamw_flat_seg_stats_(self.bucket.flat_param, self.bucket.flat_grad, self.exp_avg, self.exp_avg_sq, segs, stats,
                                  betas=self.betas, eps=self.eps, seg_counter=cnt, skip_counters=self._counters,
                                  skip_nonfinite=skip_nonfinite)
        self.last_grad_stats = stats
        return stats

    def _step_plain(self, grad_scale: float = 1.0):
        self._sync_from_group()
        self.bucket.finalize()   # pending deferred weight-gradient reductions (FactorBucket.attach)
        self._check_layout()
        if self._groups is not None:
            segs = self.segments()
            ops.adamw_flat_seg_(self.bucket.flat_param, self.bucket.flat_grad, self.exp_avg, self.exp_avg_sq, segs,
                                betas=self.betas, eps=self.eps, grad_scale=grad_scale)
            self.group_steps = [s + 1 for s in self.group_steps]
            self.step_count += 1
            return
        self.step_count += 1
        ops.adamw_flat_(self.bucket.flat_param, self.bucket.flat_grad, self.exp_avg, self.exp_avg_sq, lr=self.lr,
                        betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, step=self.step_count,
                        grad_scale=grad_scale)

    def reset_state(self, group_id=None):
        """reset_optimizer for the factor group (training_utils.py:257-277) as one launch.  group_id: zero the moments of
        that param group only (its ranges of exp_avg and exp_avg_sq, ONE sow_zero_state call) and set its step to 0 --
        the reference resets the factor group and leaves the bias group's state and step alone."""
        if group_id is None:
            ops.zero_([self.exp_avg, self.exp_avg_sq] + ([self._counters] if self._counters is not None else []))
            self.step_count = 0
            if self._groups is not None:
                self.group_steps = [0] * len(self._groups)
            return
        if self._groups is None or not 0 <= int(group_id) < len(self._groups):
            raise ValueError(f"FactorAdamW.reset_state: no param group {group_id}")
        views = []
        for gi, b, e in self._group_ranges():
            if gi == int(group_id):
                views += [self.exp_avg[b:e], self.exp_avg_sq[b:e]]
        if self._counters is not None:     # the group's skipped steps go with its step count, in the same launch
            views.append(self._counters[int(group_id):int(group_id) + 1])
        ops.zero_(views)
        self.group_steps[int(group_id)] = 0

    # ---- checkpoint / scheduler surface (simple_train.py:182, 537-563 save and restore optimizer + scheduler state)
    @property
    def param_groups(self):
        """One group, torch.optim style -- or the groups the optimizer was built with.  A driver's own scheduler code
        (`for g in opt.param_groups: g["lr"] = lr`) works on them: step() and state_dict() read the groups' values.
        torch.optim.lr_scheduler classes insist on a real torch.optim.Optimizer instance and do not accept this object --
        drive the factor lr from the loop instead (the reference computes its schedule with a LambdaLR over the torch
        optimizer; read `scheduler.get_last_lr()` and write it here)."""
        if self._groups is not None:
            return self._groups
        if not hasattr(self, "_group"):
            self._group = {"params": self.bucket.params, "lr": self.lr, "betas": self.betas, "eps": self.eps,
                           "weight_decay": self.weight_decay}
        else:
            self._sync_from_group()
        return [self._group]

    def zero_grad(self, set_to_none: bool = False):
        self.bucket.zero_grad()

    def state_dict(self):
        self._sync_from_group()
        self._fold_counters()
        sd = {"step": self.step_count, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
              "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay,
              "numel": self.bucket.padded_numel}
        if self._groups is not None:
            sd["group_lr"] = [float(g["lr"]) for g in self._groups]
            sd["group_weight_decay"] = [float(g["weight_decay"]) for g in self._groups]
            sd["group_steps"] = list(self.group_steps)
        return sd

    def load_state_dict(self, sd):
        if int(sd["numel"]) != self.bucket.padded_numel:
            raise ValueError("FactorAdamW.load_state_dict: the checkpoint belongs to a different factor layout")
        if self._groups is not None and "group_steps" in sd and len(sd["group_steps"]) != len(self._groups):
            raise ValueError("FactorAdamW.load_state_dict: the checkpoint has a different number of param groups")
        self.step_count = int(sd["step"])
        if self._counters is not None:
            self._counters.zero_()
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.lr, self.betas, self.eps, self.weight_decay = float(sd["lr"]), tuple(sd["betas"]), float(sd["eps"]), float(sd["weight_decay"])
        if hasattr(self, "_group"):
            self._group.update(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        if self._groups is not None:
            if "group_steps" in sd:
                for g, lr, wd in zip(self._groups, sd["group_lr"], sd["group_weight_decay"]):
                    g["lr"], g["weight_decay"] = float(lr), float(wd)
                self.group_steps = [int(s) for s in sd["group_steps"]]
            else:   # a one-group checkpoint: its hyper-parameters and step for every group
                for g in self._groups:
                    g["lr"], g["weight_decay"] = self.lr, self.weight_decay
                self.group_steps = [self.step_count] * len(self._groups)
            for g in self._groups:
                g["betas"], g["eps"] = self.betas, self.eps


def clip_grad_norm_(factor_opt: FactorAdamW, other_parameters, max_norm: float, *, grad_scale: float = 1.0, loss_scale=None,
                    found_inf=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (simple_train.py:631, the Trainer's max_grad_norm) for a model whose factors live in a
    FactorBucket and whose other parameters are ordinary tensors: ONE global 2-norm over both, on the device.  The squared
    norm of the other gradients is taken with torch (in float64) and enters the bucket's record as extra_sq_norm; the other gradients
    are multiplied by the record's clip_coef in place (torch._foreach_mul_ with the device scalar); flat_grad is NOT
    touched -- the record is armed on factor_opt and its next step() multiplies by grad_mult inside the AdamW kernel,
    exactly once.  grad_scale and loss_scale apply to the bucket's gradient only (the other gradients are taken as they
    are: unscale them first); the grad_scale given here is the one the armed step uses.  Returns total_norm, a 0-dim device
    tensor; nothing synchronises."""
    grads = [p.grad for p in ([other_parameters] if isinstance(other_parameters, torch.Tensor) else other_parameters)
             if p.grad is not None]
    bucket = factor_opt.bucket
    from . import ops
    ops._need_gpu(bucket.flat_grad, *grads)
    extra = None
    if grads:
        extra = torch.stack(torch._foreach_norm(grads, 2.0, dtype=torch.float64)).square().sum()   # accumulated in double
    st = bucket.grad_stats(grad_scale=grad_scale, max_norm=max_norm, extra_sq_norm=extra, loss_scale=loss_scale,
                           found_inf=found_inf)
    if grads:
        torch._foreach_mul_(grads, st.clip_coef)
    st.grad_scale = float(grad_scale)
    factor_opt.arm_grad_stats(st)
    return st.total_norm
