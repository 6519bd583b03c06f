"""Grouped execution of sibling SoWLinear layers -- the module-level face of sow_forward_group / sow_backward_group.

An HF decoder block calls `q_proj(h)`, `k_proj(h)`, `v_proj(h)` (and `gate_proj(h)`, `up_proj(h)`) one after the other
on the SAME hidden state (the reference swaps each of them for a SoWLinear, prepare.py:98-168, and the model code calls
sow.py:107-126 three times).  The layers are independent, so on MI355X they share one grid per kernel (DESIGN.md
section 4: a launch costs ~8 us of ramp and write drain whatever its size).  `group_siblings(model)` arranges that without
touching the model code: the first sibling that sees a new input computes the whole group through ONE autograd node and
parks the other outputs; the other siblings, called with the same tensor, pick theirs up.  Every layer runs its own
workgroups unchanged, so outputs and weight gradients for given inputs are bit-identical to the ungrouped calls; only the
SUM of the siblings' input gradients may round differently from autograd's own accumulation.  A sibling called with a
different input, or a group that the batched path does not cover, simply runs on its own.

`group_siblings(model, shared_input=True)` goes one step further where the kernels admit the set (bf16 / f16 parameters, no
accumulator, rank <= 64, more than 8192 tokens): the backward returns ONE input gradient, summed over the siblings in fp32
inside the kernel and rounded once (sow_backward_shared) -- no separate per-sibling input gradients and no adds (q + k + v of
llama_60m: 78.3 -> 43.9 us per backward data pass).  Outputs and weight gradients stay bit-identical
to the grouped path; the input gradient rounds differently (once instead of per sibling and per add).  The forward keeps
the grouped launch: the shared-input forward (sow_forward_shared, ops.SharedInputGroup) moves fewer bytes but measures
no faster on the llama_60m shapes (q + k + v 43.2 against 42.4 us).  A set the fused kernels do not admit runs the grouped
path unchanged.

Siblings that all carry a LOW-RANK accumulator -- the state of a from-scratch pretraining run between its first accumulate()
and the dense accumulator -- take the shared data gradient too, where their calls hold the SOW_FUSE_ACC permission
(ops.fuse_acc_default: at least 32768 tokens, widths up to 1376) and the library admits the set (ops.shared_fused_acc_admits):
ONE kernel runs every sibling's fused accumulator + live chain over a token block and sums the input gradients on chip
(chain_shared_acc.hip), dX = rn(sum_i (rn(dY_i R_i^T) Q_i^T + rn(s_i dY_i B_i^T) A_i^T)) with one rounding, instead of one
fused pass per sibling and the adds of _input_grad.  Measured at T = 32768, r = 50 (profiles/shared_fused_acc.txt): q + k + v
at r_acc = 50 128 -> 80 us, gate + up at r_acc = 50 / 100 123 -> 97 / 137 -> 114 us.  Sets whose LDS plan allows only one
workgroup per CU measured SLOWER (q + k + v at r_acc = 100 / 200: 1.12 / 1.18 of the grouped path, gate + up at 200: 1.36)
and keep the grouped path (ops.shared_fused_acc_pays).  The forward of such sets is the grouped launch, as for every set.
Siblings past 256 accumulator + live columns hold the SOW_FUSE_ACC_DEEP permission instead (ops.acc_permission); the shared
entry points ignore it, so such sets run the grouped path, one deep pass per sibling (chain_deep_acc.hip).
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib, ops
from .layer import SoWLinear, _fuse_acc, autocast_compute_dtype, autocast_input

DEFAULT_GROUPS = (("q_proj", "k_proj", "v_proj"), ("gate_proj", "up_proj"),        # Llama (simple_train.py / finetune.py targets)
                  ("query", "key", "value"))                                       # RoBERTa self-attention (run_glue.py:572)


class _SoWGroupFunction(torch.autograd.Function):
    """y_i = SoWLinear_i(x) for n layers on one input.  Tensor arguments per layer: A, B, acc_down, acc_up, bias.  cdt: the
    compute dtype of fp32 layers under torch.autocast (SOW_PARAM_F32), or None.  shared: try the shared-input data
    gradient first (group_siblings(shared_input=True))."""

    @staticmethod
    def forward(ctx, x, scales, sinks, cdt, shared, *tensors):
        n = len(scales)
        ctx.sinks = sinks
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        mixed = cdt is not None
        if mixed:
            x2 = autocast_input(x2, cdt)     # an fp32 input is cast once for the whole group
        per = [tensors[5 * i:5 * i + 5] for i in range(n)]
        need_bwd = any(ctx.needs_input_grad)
        # inside sow_amd.short_rows and sow_amd.short_codes: every sibling quantised in ONE format and admitted by its pays_short
        # rule -> one sow_forward_short_codes call on the codes read in place, no image and no arena
        ctx.short = ctx.codes = False
        if not mixed and sinks is None and n <= ops.SKINNY_MAX_LAYERS and len({getattr(t[2], "dtype", None) for t in per}) == 1 and all(
                ops.short_codes_admits(x2, A, B, acc_down, acc_up, bias) for A, B, acc_down, acc_up, bias in per):
            res = ops.sow_forward_short_codes([(x2, A, B, (acc_down, acc_up), bias, s) for (A, B, acc_down, acc_up, bias), s in zip(per, scales)],
                                              save_h=need_bwd)
            if res is not None:
                ys, hs = res
                ctx.codes, ctx.shared = True, shared
                if need_bwd:
                    ctx.save_for_backward(x2, *hs, *tensors)
                ctx.scales, ctx.n, ctx.x_shape, ctx.x_dtype, ctx.mixed = scales, n, x.shape, x.dtype, mixed
                return tuple(y.reshape(*lead, y.shape[1]) for y in ys)
        # E4M3 accumulators (codes, exponents): the siblings' images side by side in the scratch arena; the codes are what is
        # saved, backward builds the images again
        accs = ops.acc_operands([(t[2], t[3]) for t in per], x2.dtype)
        # inside sow_amd.short_rows: every sibling admitted (dense accumulators or images, the measured rule) -> one
        # sow_forward_short call for the set; sinks and autocast keep the grouped path
        if not mixed and sinks is None and n <= ops.SKINNY_MAX_LAYERS and all(
                ops.short_admits(x2, A, B, acc_down, acc_up, bias) for (A, B, _, _, bias), (acc_down, acc_up) in zip(per, accs)):
            res = ops.sow_forward_short([(x2, A, B, acc_down, bias, s) for (A, B, _, _, bias), (acc_down, _), s in zip(per, accs, scales)],
                                        save_h=need_bwd)
            if res is not None:
                ys, hs = res
                ctx.short, ctx.shared = True, shared
                if need_bwd:
                    ctx.save_for_backward(x2, *hs, *tensors)
                ctx.scales, ctx.n, ctx.x_shape, ctx.x_dtype, ctx.mixed = scales, n, x.shape, x.dtype, mixed
                return tuple(y.reshape(*lead, y.shape[1]) for y in ys)
        calls = []
        for (A, B, _, _, bias), (acc_down, acc_up), s in zip(per, accs, scales):
            kind = ops.acc_kind(acc_down, acc_up)
            calls.append(ops.LayerCall(x2, A.contiguous(), B.contiguous(),
                                       acc_down=acc_down.contiguous() if kind != _lib.ACC_NONE else None,
                                       acc_up=acc_up.contiguous() if kind == _lib.ACC_LOWRANK else None,
                                       bias=bias, scale=s, forward_only=True, save_h=need_bwd, param_f32=mixed,
                                       fuse_acc=_fuse_acc(x2, B, acc_down, acc_up, mixed)))
        ops.LayerGroup(calls).forward()   # (the shared-input forward does not pay on these shapes: module docstring)
        ctx.shared = shared
        if need_bwd:
            ctx.save_for_backward(x2, *[c.h for c in calls], *tensors)
        ctx.scales, ctx.n, ctx.x_shape, ctx.x_dtype, ctx.mixed = scales, n, x.shape, x.dtype, mixed
        return tuple(c.y.reshape(*lead, c.y.shape[1]) for c in calls)

    @staticmethod
    def _short_backward(ctx, x2, hs, tensors, dys, codes: bool):
        """The siblings' data gradients in one sow_backward_short call (codes: sow_backward_short_codes on the (codes, scales) pairs),
        then each layer's weight phases on its workspace."""
        layers = []
        for i in range(ctx.n):
            A, B, acc_down, acc_up, bias = tensors[5 * i:5 * i + 5]
            dy, d_out = dys[i], B.shape[1]
            dy2 = torch.zeros(x2.shape[0], d_out, dtype=x2.dtype, device=x2.device) if dy is None else dy.reshape(-1, d_out).contiguous()
            layers.append((dy2, x2, hs[i], A, B, (acc_down, acc_up) if codes else acc_down, ctx.scales[i], bias is not None))
        res = (ops.sow_backward_short_codes if codes else ops.sow_backward_short)(layers)
        dx = res[-1][0]        # (summed last sibling first: _input_grad)
        for g in reversed(res[:-1]):
            dx = dx + g[0]
        grads = []
        for (_, dA, dB, dbias) in res:
            grads += [dA, dB, None, None, dbias]
        return (dx.reshape(ctx.x_shape), None, None, None, None, *grads)

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        saved = ctx.saved_tensors
        x2, hs, tensors = saved[0], saved[1:1 + n], list(saved[1 + n:])
        if ctx.codes:      # (the codes as saved: no image is built)
            return _SoWGroupFunction._short_backward(ctx, x2, hs, tensors, dys, True)
        for i, (acc_down, acc_up) in enumerate(ops.acc_operands([(tensors[5 * i + 2], tensors[5 * i + 3]) for i in range(n)],
                                                                x2.dtype)):
            tensors[5 * i + 2], tensors[5 * i + 3] = acc_down, acc_up
        sinks = ctx.sinks
        if ctx.short:
            return _SoWGroupFunction._short_backward(ctx, x2, hs, tensors, dys, False)
        if sinks is not None and x2.shape[0] > 0 and all(
                s.usable(tensors[5 * i], tensors[5 * i + 1], tensors[5 * i + 4]) for i, s in enumerate(sinks)):
            # FactorBucket.attach(): ONE data-gradient launch for the siblings, weight gradients queued with their decoder
            # block (dp._GradSink); autograd gets None for the factors and for biases that are bucket members (the data
            # phase below writes no weight gradient: its dbias stays None)
            recs = []
            for i, sink in enumerate(sinks):
                A, B, acc_down, acc_up, _ = tensors[5 * i:5 * i + 5]
                kind, r_acc = sink.prepare(x2, B, acc_down, acc_up)
                T, d_out = x2.shape[0], B.shape[1]
                dy = dys[i]
                dy2 = (torch.zeros(T, d_out, dtype=x2.dtype, device=x2.device) if dy is None else dy.reshape(-1, d_out).contiguous())
                recs.append((sink, dy2, A, B, acc_down, acc_up, kind, r_acc))

            def data_calls(dxs, grad_beta):
                return [ops.LayerCall(x2, A, B, acc_down=acc_down if kind != _lib.ACC_NONE else None,
                                      acc_up=acc_up if kind == _lib.ACC_LOWRANK else None, scale=ctx.scales[i], h=hs[i],
                                      dy2=dy2, dx=dxs[i], out=(sink.pA.grad, sink.pB.grad, None), grad_beta=grad_beta, y=dy2,
                                      workspace=sink.ws, param_f32=ctx.mixed,
                                      fuse_acc=_fuse_acc(x2, B, acc_down, acc_up, ctx.mixed))
                        for i, (sink, dy2, A, B, acc_down, acc_up, kind, r_acc) in enumerate(recs)]

            # the DATA phase writes no weight gradient: grad_beta = 0 of the shared call only means dX is overwritten
            dx = _SoWGroupFunction._shared_data(ctx, x2, data_calls, n)
            if dx is None:
                calls = data_calls([torch.empty_like(x2) for _ in range(n)], 1.0)
                ops.LayerGroup(calls).backward(_lib.BWD_DATA)
                dx = _SoWGroupFunction._input_grad(ctx, calls)
            for i, (sink, dy2, A, B, acc_down, acc_up, kind, r_acc) in enumerate(recs):
                sink.queue(dy2, x2, hs[i], A, B, acc_down, acc_up, ctx.scales[i], kind, r_acc)
            return (dx, None, None, None, None, *([None] * (5 * n)))
        outs, dy2s = [], []
        for i in range(n):
            A, B, acc_down, acc_up, bias = tensors[5 * i:5 * i + 5]
            T, d_out = x2.shape[0], B.shape[1]
            dy = dys[i]
            dy2s.append(torch.zeros(T, d_out, dtype=x2.dtype, device=x2.device) if dy is None
                        else dy.reshape(-1, d_out).contiguous())
            outs.append((torch.empty_like(A), torch.empty_like(B), torch.empty_like(bias) if bias is not None else None))

        def make_calls(dxs):
            calls = []
            for i in range(n):
                A, B, acc_down, acc_up, bias = tensors[5 * i:5 * i + 5]
                kind = ops.acc_kind(acc_down, acc_up)
                calls.append(ops.LayerCall(x2, A.contiguous(), B.contiguous(),
                                           acc_down=acc_down.contiguous() if kind != _lib.ACC_NONE else None,
                                           acc_up=acc_up.contiguous() if kind == _lib.ACC_LOWRANK else None,
                                           bias=bias, scale=ctx.scales[i], h=hs[i], dy2=dy2s[i], dx=dxs[i], out=outs[i],
                                           grad_beta=0.0, y=dy2s[i], param_f32=ctx.mixed,   # y is not written by backward
                                           fuse_acc=_fuse_acc(x2, B, acc_down, acc_up, ctx.mixed)))
            return calls

        dx = None
        if ctx.shared:
            shared_dx = torch.empty_like(x2)
            if ops.SharedInputGroup(make_calls([shared_dx] * n), measured_only=True).backward(_lib.BWD_DATA | _lib.BWD_WEIGHTS):
                dx = _SoWGroupFunction._cast_input_grad(ctx, shared_dx)
        if dx is None:
            calls = make_calls([torch.empty_like(x2) for _ in range(n)])
            ops.LayerGroup(calls).backward(_lib.BWD_DATA | _lib.BWD_WEIGHTS)
            dx = _SoWGroupFunction._input_grad(ctx, calls)
        grads: List[Optional[torch.Tensor]] = []
        for (dA, dB, dbias) in outs:
            grads += [dA, dB, None, None, dbias]
        return (dx, None, None, None, None, *grads)

    @staticmethod
    def _shared_data(ctx, x2, data_calls, n):
        """The data phase through the shared-input kernel: the one input gradient, or None when the set is not admitted."""
        if not ctx.shared:
            return None
        dx = torch.empty_like(x2)
        if not ops.SharedInputGroup(data_calls([dx] * n, 0.0), measured_only=True).backward(_lib.BWD_DATA):
            return None
        return _SoWGroupFunction._cast_input_grad(ctx, dx)

    @staticmethod
    def _cast_input_grad(ctx, dx):
        return (dx if dx.dtype == ctx.x_dtype else ops.cast(dx, ctx.x_dtype)).reshape(ctx.x_shape)

    @staticmethod
    def _input_grad(ctx, calls):
        """The siblings share x: its gradient is the sum of theirs.  Summed last sibling first -- the order in which autograd
        accumulates the contributions of separately called layers (nodes run in reverse creation order), so the rounding
        matches the ungrouped model as closely as it can.  An fp32 input under autocast gets each sibling's gradient cast to
        fp32 first, as the ungrouped layers return it."""
        dxs = [c.dx if c.dx.dtype == ctx.x_dtype else ops.cast(c.dx, ctx.x_dtype) for c in calls]
        dx = dxs[-1]
        for d in reversed(dxs[:-1]):
            dx = dx + d
        return dx.reshape(ctx.x_shape)


_PER_LAYER = object()      # SiblingGroup._forward_skinny: the siblings run as single layers


class SiblingGroup:
    """SoWLinear layers of one parent module that the model calls with the same input tensor."""

    def __init__(self, layers: Sequence[SoWLinear], shared_input: bool = False):
        self.layers = list(layers)
        self.shared_input = bool(shared_input)
        self._key = None
        self._x = None                 # keeps the input alive while outputs are parked (no id() reuse)
        self._parked: dict = {}

    def usable(self, x: torch.Tensor, cdt: Optional[torch.dtype] = None) -> bool:
        """cdt: the compute dtype of fp32 layers under torch.autocast (SoWLinear's autocast_compute_dtype), or None."""
        if not x.is_cuda or x.dtype not in ops._DT:
            return False
        sinks = [getattr(m, "_grad_sink", None) for m in self.layers]
        if any(s is not None for s in sinks) and not all(s is not None for s in sinks):
            return False           # some siblings attached to a FactorBucket, some not: every layer runs on its own
        if cdt is not None and x.dtype not in (torch.float32, cdt):
            return False
        pdt = torch.float32 if cdt is not None else x.dtype
        forms = set()          # fp32 factors: the accumulators a grouped call takes are all fp32 or all native (SOW_ACC_NATIVE)
        for m in self.layers:
            if m.n_iter != 1 or m.downscale_weights[0].dtype != pdt or m.upscale_weights[0].dtype != pdt or (
                    m.bias is not None and m.bias.dtype != pdt):
                return False
            # an accumulator the grouped launch cannot take as it stands (dtype / shape / device of a checkpoint that was
            # loaded in another precision, load_sow): the layer runs on its own and raises exactly what the ungrouped
            # call raises
            try:
                kind, _ = ops.check_accumulator(x, m.in_features, m.out_features, *m._acc_pair(),
                                                param_dtype=pdt if cdt is not None else None, compute_dtype=cdt)
            except (TypeError, ValueError, RuntimeError):
                return False
            if cdt is not None and kind != _lib.ACC_NONE:
                forms.add(m.acc_downweight.dtype == torch.float32)
        return len(forms) <= 1

    def _forward_skinny(self, x: torch.Tensor, cdt: Optional[torch.dtype] = None):
        """The siblings' outputs of a generation-sized no-grad call (at most 32 flattened tokens) through ONE
        sow_forward_skinny call -- two launches for q / k / v -- or None: a set the skinny forward does not admit (any
        sibling: low-rank accumulator, wide rank, ragged widths) or that the library refuses runs the grouped path.  _PER_LAYER:
        every sibling is admitted, but their dense accumulators are of differing kinds.  cdt: the compute dtype of fp32 layers
        under autocast (absent, native and quantised accumulators are admitted there; an fp32 accumulator is not)."""
        x2 = x.reshape(-1, x.shape[-1])
        if not 1 <= x2.shape[0] <= ops.skinny_rows_limit():      # (32, or up to 64 inside sow_amd.skinny_rows)
            return None
        if cdt is not None:      # fp32 master factors under autocast: the input in the compute dtype, cast once for the set
            x2 = autocast_input(x2.contiguous(), cdt)
        calls, kinds = [], set()
        for m in self.layers:
            A, B = m.downscale_weights._parameters["0"], m.upscale_weights._parameters["0"]
            acc_down, acc_up = m._acc_pair()
            if not ops.skinny_admits(x2, A, B, acc_down, acc_up, m.bias, mixed=cdt is not None):
                return None
            calls.append((x2, A, B, ops.skinny_acc(acc_down, acc_up), m.bias, float(m.scale)))
            kinds.add(ops.acc_kind(acc_down, acc_up))
        if len(kinds - {_lib.ACC_NONE}) > 1:
            # quantised accumulators of differing formats, or quantised and unquantised ones, in one set: the library takes one
            # kind per call, and every sibling is admitted on its own -- each streams its own accumulator in a call of its own
            return _PER_LAYER
        ys = (ops.sow_forward_skinny_rows if x2.shape[0] > ops.SKINNY_MAX_T else ops.sow_forward_skinny)(calls)
        if ys is None:
            return None
        return [y.reshape(*x.shape[:-1], y.shape[1]) for y in ys]

    def forward(self, layer: SoWLinear, x: torch.Tensor) -> Optional[torch.Tensor]:
        key = (id(x), x._version, x.data_ptr(), tuple(x.shape), torch.is_grad_enabled(), torch.is_autocast_enabled("cuda"),
               torch.get_autocast_dtype("cuda"))
        if self._key == key and id(layer) in self._parked:
            y = self._parked.pop(id(layer))
            if not self._parked:
                self._key = self._x = None
            return y
        try:
            cdt = autocast_compute_dtype(layer.downscale_weights[0].dtype)
        except TypeError:
            return None            # the layer raises on its own
        if not self.usable(x, cdt):
            return None
        if not torch.is_grad_enabled():
            ys = self._forward_skinny(x, cdt)
            if ys is _PER_LAYER:
                return None
            if ys is not None:
                self._key, self._x = key, x
                self._parked = {id(m): y for m, y in zip(self.layers, ys) if m is not layer}
                return ys[self.layers.index(layer)]
        tensors = []
        for m in self.layers:
            tensors += [m.downscale_weights._parameters["0"], m.upscale_weights._parameters["0"], *m._acc_pair(), m.bias]
        sinks = tuple(getattr(m, "_grad_sink", None) for m in self.layers)
        ys = _SoWGroupFunction.apply(x, tuple(float(m.scale) for m in self.layers), sinks if sinks[0] is not None else None,
                                     cdt, self.shared_input, *tensors)
        self._key, self._x = key, x
        self._parked = {id(m): y for m, y in zip(self.layers, ys) if m is not layer}
        return ys[self.layers.index(layer)]


def group_siblings(model: nn.Module, groups: Iterable[Sequence[str]] = DEFAULT_GROUPS, shared_input: bool = False) -> int:
    """Group sibling SoWLinear layers (same parent, same in_features, one factor pair) that the model calls on the same
    input.  Returns the number of groups installed.  `ungroup_siblings(model)` removes them.  shared_input=True: the
    backward returns one input gradient, summed in the kernel, where the shared-input kernels admit the group (see the
    module docstring); otherwise the group runs exactly as with shared_input=False."""
    n = 0
    for parent in model.modules():
        for names in groups:
            mods = [getattr(parent, nm, None) for nm in names]
            if (all(isinstance(m, SoWLinear) for m in mods) and len({m.in_features for m in mods}) == 1
                    and all(m.n_iter == 1 for m in mods)):
                g = SiblingGroup(mods, shared_input=shared_input)
                for m in mods:
                    m._sibling_group = g
                n += 1
    return n


def ungroup_siblings(model: nn.Module) -> None:
    for m in model.modules():
        if isinstance(m, SoWLinear) and hasattr(m, "_sibling_group"):
            del m._sibling_group
