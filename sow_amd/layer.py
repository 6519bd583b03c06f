"""SoWLinear / SoWParameter -- host-side mirror of tn_gradient/layer/sow.py (reference lines cited per
method) whose arithmetic runs in libsow_amd.so.

Same constructor signature, attribute names and state-dict keys as the reference
(`acc_upweight`, `acc_downweight`, `downscale_weights.{i}`, `upscale_weights.{i}`, `bias`), so the
training drivers (`simple_train.py`, `finetune.py`) need no change.  Parameters stay ordinary
nn.Parameters (AdamW, DDP, save_pretrained, gradient checkpointing keep working).
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import ops


class SoWParameter(nn.ParameterList):
    """n_iter factor matrices [in_features, out_features] (reference sow.py:15-42)."""

    def __init__(self, in_features: int, out_features: int, n_iter: int = 1, device=None, dtype=None) -> None:
        kw = {"device": device, "dtype": dtype}
        super().__init__([nn.Parameter(torch.empty(in_features, out_features, **kw)) for _ in range(n_iter)])
        self.in_features = in_features
        self.out_features = out_features
        self.n_iter = n_iter

    def from_weights(self, weights: List[torch.Tensor]) -> None:
        # rebinding .data keeps the Parameter objects (optimizer / DDP references survive), sow.py:37-39
        for i, w in enumerate(weights):
            self[i].data = w.data

    def extra_repr(self) -> str:
        return f"{self.n_iter} x ({self.in_features}, {self.out_features})"


def autocast_compute_dtype(param_dtype: torch.dtype) -> Optional[torch.dtype]:
    """The compute dtype of a SoW call with parameters of `param_dtype` under torch.autocast("cuda"): bf16 / f16 for fp32
    parameters (fp32 master factors, the mixed-precision path: include/sow_amd.h SOW_PARAM_F32), None outside autocast or
    when the parameters are already of the autocast dtype (the plain path).  Other combinations raise TypeError."""
    if not torch.is_autocast_enabled("cuda"):
        return None
    ad = torch.get_autocast_dtype("cuda")
    if ad not in ops._HALF:
        raise TypeError(f"SoWLinear under torch.autocast: autocast dtype {ad} is not supported (bfloat16 or float16)")
    if param_dtype == ad:
        return None
    if param_dtype != torch.float32:
        raise TypeError(f"SoWLinear under torch.autocast({ad}): {param_dtype} parameters are not supported (float32 master "
                        f"parameters, or parameters already in {ad})")
    return ad


def autocast_input(x2: torch.Tensor, cdt: torch.dtype) -> torch.Tensor:
    """The input of a mixed-precision call in the compute dtype: fp32 is cast by the library (sow_cast_copy), as autocast
    casts the input of F.linear."""
    if x2.dtype == cdt:
        return x2
    if x2.dtype != torch.float32:
        raise TypeError(f"SoWLinear under torch.autocast({cdt}): input of dtype {x2.dtype} (float32 or {cdt})")
    return ops.cast(x2, cdt)


def _fuse_acc(x2, B, acc_down, acc_up, mixed: bool) -> int:
    """The permission of a module call (ops.acc_permission: SOW_FUSE_ACC, SOW_FUSE_ACC_DEEP or 0): the same answer on the
    grad and the no-grad route, so that eval and train outputs stay bit-identical."""
    kind = ops.acc_kind(acc_down, acc_up)
    if kind != ops._lib.ACC_LOWRANK or acc_down.dim() != 2:     # (an E4M3 accumulator is dense: no permission)
        return 0
    return ops.acc_permission(x2.shape[0], x2.shape[1], B.shape[1], B.shape[0], acc_down.shape[1], kind, x2.dtype, mixed)


class _SoWFunction(torch.autograd.Function):
    """y = acc_term + scale * (x @ A) @ B + bias through sow_forward / sow_backward (include/sow_amd.h).  cdt: the compute
    dtype of a mixed-precision call (fp32 parameters, SOW_PARAM_F32) or None."""

    @staticmethod
    def forward(ctx, x, A, B, acc_down, acc_up, bias, scale, sink=None, cdt=None):
        lead = x.shape[:-1]
        # the kernels take dense row-major buffers: a strided view (x = big[..., :d], seq[:, 0, :], W.t()) is packed ONCE
        # here so that forward and backward read the same rows (backward passes raw pointers of the saved tensors)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        if cdt is not None:
            x2 = autocast_input(x2, cdt)
        A, B = A.contiguous(), B.contiguous()
        if acc_down is not None and acc_down.numel():
            acc_down = acc_down.contiguous()
        if acc_up is not None and acc_up.numel():
            acc_up = acc_up.contiguous()
        # a low-rank accumulator and the live term in one pass where the library admits it and it measures faster
        fuse = _fuse_acc(x2, B, acc_down, acc_up, cdt is not None)
        # an E4M3 accumulator (codes, exponents): the dense kernels run on its image in the scratch arena; what is saved
        # below is the codes, and backward builds the image again
        # inside sow_amd.short_rows and sow_amd.short_codes: a quantised accumulator the format's pays_short rule keeps is read in
        # place in both directions -- no image, no arena; FactorBucket sinks and autocast keep the paths below
        res = None
        if cdt is None and sink is None and ops.short_codes_admits(x2, A, B, acc_down, acc_up, bias):
            res = ops.sow_forward_short_codes([(x2, A, B, (acc_down, acc_up), bias, scale)])
        ctx.codes = res is not None
        if res is None:
            (img_down, img_up), = ops.acc_operands([(acc_down, acc_up)], x2.dtype)
            # inside sow_amd.short_rows: a dense accumulator (or the image of a quantised one) at a row count the measured rule keeps
            # runs forward and data gradient on the skinny kernel pair; FactorBucket sinks and autocast keep the path below
            if cdt is None and sink is None and ops.short_admits(x2, A, B, img_down, img_up, bias):
                res = ops.sow_forward_short([(x2, A, B, img_down, bias, scale)])
        ctx.short = res is not None and not ctx.codes
        if res is not None:
            (y,), (h,) = res
        else:
            y, h = ops.sow_forward(x2, A, B, img_down, img_up, bias, scale, param_f32=cdt is not None, fuse_acc=fuse)
        ctx.fuse_acc = fuse
        ctx.save_for_backward(x2, h, A, B, acc_down, acc_up)
        ctx.scale = scale
        ctx.has_bias = bias is not None
        ctx.bias = bias           # identity only (the sink checks it is the bucket's parameter); backward reads no bias
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        ctx.sink = sink
        ctx.mixed = cdt is not None
        return y.reshape(*lead, B.shape[1])

    @staticmethod
    def backward(ctx, dy):
        x2, h, A, B, acc_down, acc_up = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        sink = ctx.sink
        if not ctx.codes:
            (acc_down, acc_up), = ops.acc_operands([(acc_down, acc_up)], x2.dtype)
        if ctx.codes:
            (dx, dA, dB, dbias), = ops.sow_backward_short_codes([(dy2, x2, h, A, B, (acc_down, acc_up), ctx.scale, ctx.has_bias)])
        elif ctx.short:
            (dx, dA, dB, dbias), = ops.sow_backward_short([(dy2, x2, h, A, B, acc_down, ctx.scale, ctx.has_bias)])
        elif sink is not None and x2.shape[0] > 0 and sink.usable(A, B, ctx.bias):
            # FactorBucket.attach(): the weight gradients accumulate straight into the flat gradient buffer (p.grad is a
            # view of it), so autograd gets None for A and B (and for a bias that is a bucket member: its gradient comes
            # out of the same partial sums); the slab-partial sums are reduced for all layers in one launch by
            # FactorBucket.finalize() (sow_reduce_batch).
            dx = sink.backward(dy2, x2, h, A, B, acc_down, acc_up, ctx.scale)
            dA = dB = dbias = None
        else:
            dx, dA, dB, dbias = ops.sow_backward(dy2, x2, h, A, B, acc_down, acc_up, ctx.scale, ctx.has_bias,
                                                 param_f32=ctx.mixed, fuse_acc=ctx.fuse_acc)
        if dx.dtype != ctx.x_dtype:
            dx = ops.cast(dx, ctx.x_dtype)      # fp32 input under autocast: its gradient, cast back by the library
        return dx.reshape(ctx.x_shape), dA, dB, None, None, dbias, None, None, None


class SoWLinear(nn.Module):
    """Sum-of-Weights low-rank linear layer (reference sow.py:45-181)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, rank: int = 16, n_iter: int = 1,
                 scale: float = 1, init_method: str = "normal_QR", device=None, dtype=None, init_params=True) -> None:
        kw = {"device": device, "dtype": dtype}
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.n_iter = n_iter
        self.rank = rank
        self.scale = scale
        self.virtual_rank = min(rank * n_iter, in_features, out_features)  # sow.py:67
        # frozen accumulator, zero-numel until the first accumulate() / prepare_sow (sow.py:69-70)
        self.acc_upweight = nn.Parameter(torch.empty(0), requires_grad=False)
        self.acc_downweight = nn.Parameter(torch.empty(0), requires_grad=False)
        self.init_method = init_method
        self.downscale_weights = SoWParameter(in_features, rank, n_iter=n_iter, device=device, dtype=dtype)
        self.upscale_weights = SoWParameter(rank, out_features, n_iter=n_iter, device=device, dtype=dtype)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features, **kw))
        else:
            self.register_parameter("bias", None)
        if init_params:
            self.reset_parameters()

    # ------------------------------------------------------------------------------------------
    def _fresh_gaussian(self, shape, device, dtype):
        w = torch.zeros(shape, device=device, dtype=dtype)
        return nn.init.normal_(w, mean=0.0, std=0.02)  # std hard-coded as in sow.py:96 / :169

    _fresh_gaussian_default = _fresh_gaussian   # lets the batched accumulate see whether a test has replaced the draw

    def reset_parameters(self, reset_scale=1.0) -> None:
        """sow.py:89-105.  normal_QR: A = Q[:, :r], B = R[:r, :] of the QR of an fp32 N(0, 0.02^2)
        [in, out] draw (the reference draws it on "cuda", :91 -- here on the factors' GPU)."""
        for i in range(self.n_iter):
            if i / self.n_iter >= 1 - reset_scale:
                a, b = self.downscale_weights[i], self.upscale_weights[i]
                if self.init_method == "normal_QR":
                    if not a.is_cuda:
                        raise RuntimeError("SoWLinear(init_method='normal_QR') initialises on the GPU "
                                           "(reference sow.py:91 hard-codes 'cuda'); construct with device='cuda'")
                    w = self._fresh_gaussian((self.in_features, self.out_features), a.device, torch.float32)
                    q, r = ops.qr_thin(w, self.rank, need_r=True, out_dtype=torch.float32)
                    self.downscale_weights[i] = q.to(a.dtype).contiguous()
                    self.upscale_weights[i] = r.to(b.dtype).contiguous()
                else:
                    nn.init.normal_(a, std=0.02)
                    nn.init.normal_(b, std=0.02)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    # ------------------------------------------------------------------------------------------
    def _cat_factors(self):
        if self.n_iter == 1:
            # direct dict access: ParameterList.__getitem__ costs ~5 us per lookup on the per-call path
            return self.downscale_weights._parameters["0"], self.upscale_weights._parameters["0"]
        # sum_i A_i B_i = [A_1 .. A_n] [B_1; ..; B_n]; autograd splits the gradients back
        return torch.cat(list(self.downscale_weights), dim=1), torch.cat(list(self.upscale_weights), dim=0)

    # ------------------------------------------------------------------------------------------
    # A dense accumulator quantised by sow_amd.quantize_accumulators: acc_downweight holds the E4M3 codes (a frozen
    # float8_e4m3fn parameter) and the persistent buffer acc_exponent the int8 column exponents -- or, for fmt="mxfp4", the packed
    # E2M1 codes (uint8 [d_in / 2, d_out]) and the uint8 E8M0 block scales [d_in / 32, d_out] (the formats: acc_format.py).  An
    # unquantised layer has no such buffer: its state-dict keys are the reference's.
    def acc_quantized(self) -> bool:
        return self._buffers.get("acc_exponent") is not None

    def _acc_pair(self):
        """(acc_down, acc_up) as the kernels' wrappers take them: the exponents ride in acc_up's place next to the codes."""
        exps = self._buffers.get("acc_exponent")
        return (self.acc_downweight, self.acc_upweight if exps is None else exps)

    def _apply(self, fn, *args, **kwargs):
        # .half() / .bfloat16() / .to(dtype) cast every floating-point parameter: the codes would become their unscaled values
        # in the new dtype.  They stay codes (moved with the module); the layer then computes in the dtype of its factors.
        codes = self.acc_downweight.data if self.acc_quantized() else None     # (the tensor: _apply rebinds the parameter's .data)
        super()._apply(fn, *args, **kwargs)
        if codes is not None and self.acc_downweight.dtype != codes.dtype:     # (uint8 MXFP4 codes are left alone by casts anyway)
            self.acc_downweight = nn.Parameter(codes.to(self.acc_downweight.device), requires_grad=False)
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a quantised state dict into an unquantised layer (or the other way round): the layer takes the form of what it loads,
        # so that strict loading sees the keys it expects and the codes are copied as codes
        # (E4M3 codes with int8 exponents, or packed MXFP4 codes with uint8 block scales)
        codes, exps = state_dict.get(prefix + "acc_downweight"), state_dict.get(prefix + "acc_exponent")
        if exps is not None and codes is not None and codes.dtype in ops.CODES and not (
                self.acc_quantized() and self.acc_downweight.dtype == codes.dtype and self.acc_downweight.shape == codes.shape
                and self.acc_exponent.dtype == exps.dtype and self.acc_exponent.shape == exps.shape):
            dev = self.acc_downweight.device
            self.acc_downweight = nn.Parameter(torch.empty(codes.shape, dtype=codes.dtype, device=dev), requires_grad=False)
            self._buffers.pop("acc_exponent", None)
            self.register_buffer("acc_exponent", torch.empty(exps.shape, dtype=exps.dtype, device=dev))
        elif exps is None and codes is not None and codes.dtype not in ops.CODES and self.acc_quantized():
            del self._buffers["acc_exponent"]
            self.acc_downweight = nn.Parameter(torch.empty(codes.shape, dtype=codes.dtype, device=self.acc_downweight.device),
                                               requires_grad=False)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """sow.py:107-126 in one fused call: accumulator term (not scaled) + scale * (x A) B + bias."""
        group = self.__dict__.get("_sibling_group")     # sow_amd.group.group_siblings: q/k/v or gate/up in one launch
        if group is not None:
            y = group.forward(self, x)
            if y is not None:
                return y
        A, B = self._cat_factors()
        acc_down, acc_up = self._acc_pair()
        # torch.autocast with fp32 factors: bf16 / f16 kernels on factors rounded once by the library, fp32 gradients
        cdt = autocast_compute_dtype(A.dtype)
        if not (torch.is_grad_enabled() and (x.requires_grad or A.requires_grad or B.requires_grad
                                             or (self.bias is not None and self.bias.requires_grad))):
            # no backward will follow (eval / generate, commonsense_evaluate.py:268-287; the first pass of activation
            # checkpointing): the projection h = scale * x A is not written to HBM
            x2 = x.reshape(-1, x.shape[-1])
            if cdt is not None:
                x2 = autocast_input(x2.contiguous(), cdt)
            # generation-sized calls (generate(): batch x beams rows per new token): the fused skinny forward, two launches,
            # the accumulator (or its E4M3 / MXFP4 codes: a half / a quarter of the bytes) streamed once on the whole chip.  Under
            # autocast with fp32 factors it takes an absent, native (compute dtype) or quantised accumulator and rounds the
            # factors in registers.  An fp32 accumulator under autocast, a low-rank accumulator, a wide rank, ragged widths and a
            # refusal from the library keep the path below.
            # Inside sow_amd.skinny_rows(n), calls of 33 ... n rows take sow_forward_skinny_rows the same way.
            if x2.shape[0] <= ops.skinny_rows_limit() and ops.skinny_admits(x2, A, B, acc_down, acc_up, self.bias, mixed=cdt is not None):
                fwd = ops.sow_forward_skinny_rows if x2.shape[0] > ops.SKINNY_MAX_T else ops.sow_forward_skinny
                ys = fwd([(x2, A, B, ops.skinny_acc(acc_down, acc_up), self.bias, float(self.scale))])
                if ys is not None:
                    return ys[0].reshape(*x.shape[:-1], B.shape[1])
            # inside sow_amd.short_rows and sow_amd.short_codes: the forward on the codes read in place, h_save = NULL
            if cdt is None and ops.short_codes_admits(x2, A, B, acc_down, acc_up, self.bias):
                res = ops.sow_forward_short_codes([(x2, A, B, (acc_down, acc_up), self.bias, float(self.scale))], save_h=False)
                if res is not None:
                    return res[0][0].reshape(*x.shape[:-1], B.shape[1])
            # every other call of a quantised layer: the existing dense path on the image
            (acc_down, acc_up), = ops.acc_operands([(acc_down, acc_up)], x2.dtype)
            # inside sow_amd.short_rows: 65 ... 1024 rows of a dense accumulator on the skinny pair, h_save = NULL
            if cdt is None and ops.short_admits(x2, A, B, acc_down, acc_up, self.bias):
                res = ops.sow_forward_short([(x2, A, B, acc_down, self.bias, float(self.scale))], save_h=False)
                if res is not None:
                    return res[0][0].reshape(*x.shape[:-1], B.shape[1])
            y, _ = ops.sow_forward(x2, A, B, acc_down, acc_up, self.bias, float(self.scale), save_h=False,
                                   param_f32=cdt is not None, fuse_acc=_fuse_acc(x2, B, acc_down, acc_up, cdt is not None))
            return y.reshape(*x.shape[:-1], B.shape[1])
        return _SoWFunction.apply(x, A, B, acc_down, acc_up, self.bias, float(self.scale), getattr(self, "_grad_sink", None), cdt)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def accumulate(self):
        """sow.py:128-178: fold scale * sum_i A_i B_i into the accumulator, optionally re-factor it by
        truncated QR, re-initialise A, zero B."""
        if self.acc_quantized():
            raise RuntimeError("SoWLinear.accumulate: the accumulator is quantised (E4M3 / MXFP4) and frozen; merging into it would "
                               "requantise it.  Call sow_amd.dequantize_accumulators(model) first")
        A = torch.cat([w.data for w in self.downscale_weights], dim=1) if self.n_iter > 1 else self.downscale_weights[0].data
        B = torch.cat([w.data for w in self.upscale_weights], dim=0) if self.n_iter > 1 else self.upscale_weights[0].data
        if not A.is_cuda:
            raise RuntimeError("SoWLinear.accumulate runs on the GPU; there is no CPU fallback")
        has_down = self.acc_downweight.numel() != 0
        has_up = self.acc_upweight.numel() != 0
        scale = float(self.scale)
        # fp32 master factors over a bf16 / f16 base: the factors fold as the forward reads them, rounded once to the
        # accumulator's dtype, and the accumulator keeps its dtype
        mixed = has_down and A.dtype == torch.float32 and self.acc_downweight.dtype in ops._HALF
        if mixed:
            A, B = A.to(self.acc_downweight.dtype), B.to(self.acc_downweight.dtype)
        if has_down and has_up:      # W_acc = Q R, then += scale * A B   (sow.py:137-138)
            acc = ops.gemm(self.acc_downweight.data.to(A.dtype), self.acc_upweight.data.to(A.dtype))
            ops.gemm(A, B, out=acc, alpha=scale, beta=1.0)
        elif has_down:               # dense accumulator updated in place (sow.py:139-140)
            acc = self.acc_downweight.data
            if mixed:
                ops.gemm(A, B, out=acc, alpha=scale, beta=1.0)
            else:
                if acc.dtype != A.dtype:
                    acc = acc.to(A.dtype)
                ops.gemm(A, B, out=acc, alpha=scale, beta=1.0)
        else:
            acc = ops.gemm(A, B, alpha=scale)

        if self.virtual_rank < min(self.in_features, self.out_features):   # sow.py:144-150
            q, r = ops.qr_thin(acc, self.virtual_rank, need_r=True)
            self.acc_downweight = nn.Parameter(q, requires_grad=False)
            self.acc_upweight = nn.Parameter(r, requires_grad=False)
            self.virtual_rank = min(self.virtual_rank + self.rank * self.n_iter, self.in_features, self.out_features)
        else:                                                              # sow.py:151-153
            self.acc_downweight = nn.Parameter(acc, requires_grad=False)
            # zero-numel placeholder as in the reference (default dtype), but on the layer's device so that a state dict
            # taken after accumulate() does not mix devices
            self.acc_upweight = nn.Parameter(torch.empty(0, device=acc.device), requires_grad=False)

        # new factors: B <- 0 (sow.py:159), A <- Q[:, :r] of a fresh Gaussian (sow.py:161-172) or a Gaussian (:174)
        new_down = [torch.zeros_like(w) for w in self.downscale_weights]
        new_up = [torch.empty_like(w) for w in self.upscale_weights]
        ops.zero_(new_up)
        for i in range(self.n_iter):
            if self.init_method == "normal_QR":
                w = self._fresh_gaussian((self.in_features, self.out_features), self.acc_downweight.device,
                                         self.acc_downweight.dtype)
                q, _ = ops.qr_thin(w, self.rank, need_r=False, out_dtype=new_down[i].dtype)   # (the factor dtype)
                new_down[i] = q.contiguous()
            else:   # plain Gaussian re-init (sow.py:174), through the same draw hook as the QR branch
                new_down[i] = self._fresh_gaussian(tuple(new_down[i].shape), new_down[i].device, new_down[i].dtype)
        self.downscale_weights.from_weights(new_down)
        self.upscale_weights.from_weights(new_up)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"rank={self.rank}, n_iter={self.n_iter}")
