"""Tensor-level wrappers over the C ABI (raw device pointers + the current HIP stream).

PyTorch is used for device memory (the caching allocator owns every buffer), the
stream and the autograd plumbing only; all arithmetic runs in libsow_amd.so.
Every function requires CUDA(=HIP) tensors and raises otherwise.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .acc_format import BY_CODE_DTYPE, BY_KIND, FORMATS, SKINNY_MAX_T, SKINNY_ROWS_MAX, skinny_fp4_pays, skinny_fp8_pays  # noqa: F401

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_HALF = (torch.bfloat16, torch.float16)
FP8, FP4 = FORMATS["fp8_e4m3"].code_dtype, FORMATS["mxfp4"].code_dtype     # the quantised formats are described in acc_format.py:
CODES, FP4_BLOCK = tuple(BY_CODE_DTYPE), FORMATS["mxfp4"].block            # these are its facts under the names tests and tools read
_NOT_A_PAIR = f"not the codes and scales of a quantised accumulator ({', '.join(FORMATS)}: their dtypes and shapes are in acc_format.py)"


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"sow_amd supports float32, bfloat16 and float16 tensors, got {t.dtype}") from None


_PERMS = _lib.FUSE_ACC | _lib.FUSE_ACC_DEEP


def _perm(fuse_acc) -> int:
    """The ONE permission value a layer call carries, as its dtype bit: 0 (none), SOW_FUSE_ACC or SOW_FUSE_ACC_DEEP.
    `fuse_acc` is that bit, or a bool with today's meaning (True = SOW_FUSE_ACC)."""
    if fuse_acc is True:
        return _lib.FUSE_ACC
    if not fuse_acc:
        return 0
    if fuse_acc not in (_lib.FUSE_ACC, _lib.FUSE_ACC_DEEP):
        raise ValueError("sow_amd: fuse_acc is a bool, _lib.FUSE_ACC or _lib.FUSE_ACC_DEEP")
    return int(fuse_acc)


def acc_native(x2: torch.Tensor, acc_down: Optional[torch.Tensor]) -> bool:
    """Whether the accumulator of a call with fp32 parameters on activations x2 is NATIVE: held in the compute dtype (x2's), so
    that the kernels read it in place (SOW_ACC_NATIVE) -- a frozen bf16 / f16 base, or the image of a quantised one."""
    return acc_down is not None and acc_down.numel() != 0 and acc_down.dtype == x2.dtype and x2.dtype != torch.float32


def _call_dtype(x2: torch.Tensor, param_f32: bool, who: str = "sow_amd", fuse_acc=False,
                acc_down: Optional[torch.Tensor] = None) -> Tuple[int, torch.dtype]:
    """(C-ABI dtype code, parameter dtype) of a layer call on activations x2.  param_f32: the parameters (factors, bias) are
    fp32 and x2 is of the compute dtype, bf16 or f16 (SOW_PARAM_F32: mixed precision, torch.autocast); the accumulator
    `acc_down` is fp32 as well (packed with them) or native (acc_native: SOW_ACC_NATIVE is set, it is read in place).
    fuse_acc: the call's permission (_perm: SOW_FUSE_ACC or SOW_FUSE_ACC_DEEP; bf16 / f16 parameters only: the library
    ignores it next to SOW_PARAM_F32, so it is not passed there)."""
    dt = _dt(x2)
    if not param_f32:
        return (dt | _perm(fuse_acc) if dt != _lib.F32 else dt), x2.dtype
    if dt == _lib.F32:
        raise TypeError(f"{who}: fp32 parameters need bfloat16 or float16 activations, got {x2.dtype}")
    return dt | _lib.PARAM_F32 | (_lib.ACC_NATIVE if acc_native(x2, acc_down) else 0), torch.float32


def _need_gpu(*ts: Optional[torch.Tensor]) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("sow_amd: the SoW hot path runs on MI355X only (got a CPU tensor); "
                               "there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"sow_amd: tensors on different devices ({dev} vs {t.device})")
    return dev


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device: Optional[torch.device] = None) -> int:
    """hipStream_t of the current torch stream.  torch.cuda.current_stream() builds a Stream object (~20 us of host
    time per call, as much as everything else in a layer call); the raw getter is ~1 us."""
    if _raw_stream is not None:
        idx = device.index if (device is not None and device.index is not None) else torch.cuda.current_device()
        return _raw_stream(idx)
    return torch.cuda.current_stream(device).cuda_stream


def _launch_rc(dev: torch.device, fn, *args) -> int:
    """Call a C-ABI launcher with the tensors' device current (the kernels run on the HIP device that is current on the
    calling thread; the stream argument is that device's current torch stream) and return its code.  One process per GPU
    never takes the slow branch; a process that touches several GPUs gets the right device instead of an invalid-handle
    error."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx == torch.cuda.current_device():
        return fn(*args, _stream(dev))
    with torch.cuda.device(idx):
        return fn(*args, _stream(dev))


def _launch(dev: torch.device, what: str, fn, *args) -> None:
    """_launch_rc for the callers that take any non-zero code as an error."""
    _lib.check(_launch_rc(dev, fn, *args), what)


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


_WS_BYTES: dict = {}
_GEMM_WS_BYTES: dict = {}
_FWD_WS_BYTES: dict = {}


def _forward_workspace_bytes(lib, T: int, d_in: int, d_out: int, r: int, r_acc: int, kind: int, dt: int) -> int:
    """sow_forward_workspace_bytes (0 for most shapes), memoised per shape."""
    key = (T, d_in, d_out, r, r_acc, kind, dt)
    n = _FWD_WS_BYTES.get(key)
    if n is None:
        n = _FWD_WS_BYTES[key] = int(lib.sow_forward_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt))
    return n


def _workspace_bytes(lib, T: int, d_in: int, d_out: int, r: int, r_acc: int, kind: int, dt: int) -> int:
    """sow_workspace_bytes, memoised per shape (a ctypes round trip per layer call otherwise)."""
    key = (T, d_in, d_out, r, r_acc, kind, dt)
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = int(lib.sow_workspace_bytes(T, d_in, d_out, r, r_acc, kind, dt))
    return n


def _acc_kind_fmt(acc_down, acc_up):
    """(kind, format record or None): the ONE place that tells a quantised accumulator from the others, by its codes' dtype."""
    if acc_down is None or acc_down.numel() == 0:
        return _lib.ACC_NONE, None
    fmt = BY_CODE_DTYPE.get(acc_down.dtype)
    if fmt is not None:
        return fmt.kind, fmt
    return (_lib.ACC_DENSE if acc_up is None or acc_up.numel() == 0 else _lib.ACC_LOWRANK), None


def acc_kind(acc_down: Optional[torch.Tensor], acc_up: Optional[torch.Tensor]) -> int:
    """Accumulator kind as SoWLinear.forward decides it (reference sow.py:109-112); codes of a quantised format: that format's kind."""
    return _acc_kind_fmt(acc_down, acc_up)[0]


def check_accumulator(x2: torch.Tensor, d_in: int, d_out: int, acc_down, acc_up, who: str = "sow_amd",
                      param_dtype: Optional[torch.dtype] = None, compute_dtype: Optional[torch.dtype] = None) -> Tuple[int, int]:
    """(acc_kind, r_acc) after the checks every entry point applies before raw pointers reach the kernels: the
    accumulator has the input's dtype (TypeError), the shapes of its kind (ValueError), lives on the input's device and is
    dense row-major.  A mismatch that got through would be read as the wrong type -- silent garbage for an fp32
    accumulator under bf16 inputs, an out-of-bounds device read the other way round.  `param_dtype`: the parameter dtype
    of the call when it is not the input's (fp32 under SOW_PARAM_F32).  The accumulator next to fp32 parameters has one of
    three forms: fp32 (packed with the factors by every call), the compute dtype (native, read in place: SOW_ACC_NATIVE), or
    E4M3 / MXFP4 codes (run on their image in the compute dtype, or streamed by the skinny forward).  `compute_dtype`: the
    compute dtype when x2 is not of it yet (an fp32 input under autocast that the call casts first)."""
    kind, fmt = _acc_kind_fmt(acc_down, acc_up)
    cdt = x2.dtype if compute_dtype is None else compute_dtype
    if kind == _lib.ACC_NONE:
        return kind, 0
    r_acc = 0
    if fmt is not None:
        if param_dtype not in (None, torch.float32) or cdt not in _HALF:
            raise TypeError(f"{who}: an {fmt.label} accumulator runs with bfloat16 or float16 inputs and parameters, got {cdt}"
                            + ("" if param_dtype is None else f" inputs and {param_dtype} parameters"))
        if acc_up is None or acc_up.dtype != fmt.scale_dtype:
            raise TypeError(f"{who}: an {fmt.label} accumulator comes with {fmt.scale_dtype} scales")
        if (d_in % (fmt.block or 1) or d_out % fmt.d_out_multiple or tuple(acc_down.shape) != fmt.code_shape(d_in, d_out)
                or tuple(acc_up.shape) != fmt.scale_shape(d_in, d_out)):
            raise ValueError(f"{who}: an {fmt.label} accumulator of [{d_in}, {d_out}] is codes {fmt.code_shape(d_in, d_out)} and scales "
                             f"{fmt.scale_shape(d_in, d_out)}, out_features a multiple of {fmt.d_out_multiple}"
                             + (f", in_features whole blocks of {fmt.block}" if fmt.block else ""))
    else:
        want = x2.dtype if param_dtype is None else param_dtype
        if param_dtype == torch.float32 and acc_down.dtype == cdt and cdt in _HALF:
            want = cdt      # native: both tensors of the accumulator in the compute dtype
        if acc_down.dtype != want or (kind == _lib.ACC_LOWRANK and acc_up.dtype != want):
            bad = acc_down.dtype if acc_down.dtype != want else acc_up.dtype
            raise TypeError(f"{who}: dtype mismatch, x is {x2.dtype} but the accumulator is {bad}"
                            + ("" if param_dtype is None else f" (parameters must be {param_dtype}; the accumulator {param_dtype} "
                                                               f"or the compute dtype)"))
        if kind == _lib.ACC_DENSE and tuple(acc_down.shape) != (d_in, d_out):
            raise ValueError(f"{who}: dense accumulator must be [in_features, out_features]")
        if kind == _lib.ACC_LOWRANK:
            r_acc = acc_down.shape[1] if acc_down.dim() == 2 else -1
            if acc_down.dim() != 2 or acc_down.shape[0] != d_in or tuple(acc_up.shape) != (r_acc, d_out):
                raise ValueError(f"{who}: low-rank accumulator shapes do not match")
    for t in (acc_down, acc_up if kind != _lib.ACC_DENSE else None):      # (a dense accumulator has no second tensor)
        if t is not None and (not t.is_cuda or t.device != x2.device):
            raise RuntimeError(f"{who}: the accumulator is on {t.device}, the input on {x2.device}")
    return kind, r_acc


def fused_acc_admits(d_in: int, d_out: int, r: int, r_acc: int, kind: int, dtype: torch.dtype,
                     param_f32: bool = False) -> bool:
    """The admitted set of SOW_FUSE_ACC (include/sow_amd.h; fused_acc_shape_ok in the library): a bf16 / f16 layer without
    fp32 parameters, a low-rank accumulator, even r in [2, 64], even r_acc >= 2, r_acc + r <= 256, widths multiples of 8.
    The call-time conditions (16-byte-aligned tensors, the flagged workspace) hold for every tensor the module surface
    allocates."""
    return (dtype in (torch.bfloat16, torch.float16) and not param_f32 and kind == _lib.ACC_LOWRANK
            and 2 <= r <= 64 and r % 2 == 0 and r_acc >= 2 and r_acc % 2 == 0 and r_acc + r <= 256
            and d_in > 0 and d_out > 0 and d_in % 8 == 0 and d_out % 8 == 0)


FUSED_ACC_MIN_T = 32768     # the token count of profiles/lowrank_acc.txt
FUSED_ACC_MAX_D = 1376      # its widest layer (512 -> 1376, 1376 -> 512)


def fused_acc_pays(T: int, d_in: int, d_out: int, r: int, r_acc: int) -> bool:
    """The measured dispatch rule of the module surface for SOW_FUSE_ACC (profiles/lowrank_acc.txt, DESIGN.md section
    4.4e): the classes of (r_pad = ceil64(r_acc + r), shape) at which the fused pass beats the two chain launches it
    replaces, forward + data gradient together, by more than the two-pass variant's own spread.

    Measured (bf16; one f16 row), us of forward + data gradient, two-pass -> fused (two-pass spread), T = 32768:
        512->512,  r = 50, r_acc = 50 / 100 / 150 / 200 (r_pad 128 / 192 / 256 / 256): 100 -> 73 (2.5), 129 -> 82 (4.5),
                                                                                        136 -> 90 (5.0), 145 -> 90 (3.4)
        512->1376: 183 -> 110 (1.1), 215 -> 126 (6.3), 230 -> 145 (10.6), 251 -> 147 (10.8)
        1376->512: 178 -> 110 (1.2), 215 -> 127 (7.5), 232 -> 146 (10.2), 250 -> 143 (6.3)
        768->768,  r = 8, r_acc = 8 / 56 (r_pad 64): 135 -> 81 (1.0), 138 -> 82 (1.4);   f16 512->512, r_acc = 100: 128 -> 82 (2.0)
    Every class of r_pad (64, 128, 192, 256) pays at each of these shapes, by 27 to 43 %.  The rule is these rows: calls of at
    least FUSED_ACC_MIN_T tokens on layers no wider than FUSED_ACC_MAX_D -- the envelope the test suite was run with.
    Also measured, also paying (ratio 0.58 to 0.78), but outside the default until the suite has run with a wider one:
    T = 16384 at the three llama_60m shapes, and 2048 -> 2048 / 4096 -> 4096 at r_acc = 50 and 200.
    NOT measured: fewer than 16384 tokens (below 8193 the two-pass path also splits its chains over K and the output columns
    to fill the chip, launch_chain_short, and the fused pass does not), widths above 4096, r other than 8 and 50."""
    return T >= FUSED_ACC_MIN_T and max(d_in, d_out) <= FUSED_ACC_MAX_D


def fuse_acc_default(T: int, d_in: int, d_out: int, r: int, r_acc: int, kind: int, dtype: torch.dtype,
                     param_f32: bool = False) -> bool:
    """Whether the module surface passes the SOW_FUSE_ACC permission for this layer call: admitted and measured to pay."""
    return fused_acc_admits(d_in, d_out, r, r_acc, kind, dtype, param_f32) and fused_acc_pays(T, d_in, d_out, r, r_acc)


DEEP_ACC_MAX_TOT = 960                  # 15 panels of 64 columns: 120 KiB of H next to the 40 KiB stage
DEEP_ACC_MAX_LDS = 160 * 1024


def deep_acc_admits(d_in: int, d_out: int, r: int, r_acc: int, kind: int, dtype: torch.dtype,
                    param_f32: bool = False) -> bool:
    """The admitted set of SOW_FUSE_ACC_DEEP (include/sow_amd.h; deep_acc_shape_ok in the library): a bf16 / f16 layer
    without fp32 parameters, a low-rank accumulator, even r in [2, 64], even r_acc, 256 < r_acc + r <= 960, widths
    multiples of 8.  Disjoint from fused_acc_admits by the total.  The call-time conditions hold for every tensor the module
    surface allocates."""
    return (dtype in (torch.bfloat16, torch.float16) and not param_f32 and kind == _lib.ACC_LOWRANK
            and 2 <= r <= 64 and r % 2 == 0 and r_acc >= 2 and r_acc % 2 == 0 and 256 < r_acc + r <= DEEP_ACC_MAX_TOT
            and d_in > 0 and d_out > 0 and d_in % 8 == 0 and d_out % 8 == 0)


def deep_acc_lds_bytes(r_tot: int) -> int:
    """The LDS plan of chain_deep_acc.hip for r_tot = r_acc + r: 128 bytes per column of r_pad = ceil64(r_tot) and the 40
    KiB stage.  At most 80 KiB (r_pad <= 320) two workgroups share a CU."""
    return (r_tot + 63) // 64 * 64 * 128 + 40960


DEEP_ACC_MIN_T = 16384      # the shortest row of profiles/deep_acc.txt (an r_acc that is no multiple of 8)
DEEP_ACC_MIN_T_WIDE = 32768  # ... and the only token count measured where the unflagged accumulator term is chain_wide
DEEP_ACC_MAX_D = 1376       # its widest layer (512 -> 1376, 1376 -> 512)


def deep_acc_pays(T: int, d_in: int, d_out: int, r: int, r_acc: int) -> bool:
    """The measured dispatch rule of the module surface for SOW_FUSE_ACC_DEEP (profiles/deep_acc.txt, DESIGN.md section
    4.4f), the one place that encodes it: the classes at which the deep pass beats the unflagged call, forward and data
    gradient each and together, by more than the unflagged variant's own spread.  What decides is the kernel the unflagged
    accumulator term runs on, which follows from r_acc:

    Measured (bf16, r = 50, T = 32768; us of forward + data gradient, unflagged -> deep (unflagged spread)):
      r_acc <= 256 (unflagged: chain_wide + live chain; deep plans 80 KiB, two workgroups per CU), r_acc = 250:
        512->512 154 -> 132 (9.6), 512->1376 257 -> 209 (13.2), 1376->512 256 -> 209 (11.5): pays, ratio 0.81 to 0.86
      r_acc > 256, no multiple of 8 (unflagged: two launches of the generic GEMM off its vector path), r_acc = 300 / 450 / 500:
        512->512 1810 -> 225, 2338 -> 260, 2336 -> 318; 512->1376 3290 -> 385, 4383 -> 454, 4402 -> 559;
        1376->512 3393 -> 390, 4283 -> 455, 4297 -> 559; 1024->1024 at r_acc = 900 (160 KiB): 8570 -> 880;
        f16 512->512 at 300: 1807 -> 223; T = 16384, 512->1376 at 450: 2232 -> 241: pays, ratio 0.10 to 0.14
      r_acc > 256, a multiple of 8 (unflagged: the generic GEMM on its vector path), one workgroup per CU for the deep pass:
        r_acc = 400: 512->512 192 -> 246, 512->1376 320 -> 425, 1376->512 322 -> 424; 768->768 at 600: 311 -> 469;
        768->768, r = 8, r_acc = 504: 264 -> 348: LOSES, ratio 1.28 to 1.51 -- stays off
    The rule is these rows: widths up to DEEP_ACC_MAX_D; r_acc no multiple of 8 past 256 columns from DEEP_ACC_MIN_T tokens,
    r_acc <= 256 from DEEP_ACC_MIN_T_WIDE tokens; multiples of 8 past 256 never.  NOT measured, hence off: fewer tokens
    and widths above 1376.  Inside the envelope but not timed one by one: r_acc = 350 (its class, no multiple of 8, has five
    rows), r_acc <= 256 at an r other than 50."""
    if T < DEEP_ACC_MIN_T or max(d_in, d_out) > DEEP_ACC_MAX_D:
        return False
    if r_acc <= 256:
        return T >= DEEP_ACC_MIN_T_WIDE
    return r_acc % 8 != 0


def acc_permission(T: int, d_in: int, d_out: int, r: int, r_acc: int, kind: int, dtype: torch.dtype,
                   param_f32: bool = False) -> int:
    """The ONE permission the module surface passes for this layer call: _lib.FUSE_ACC (fuse_acc_default), _lib.FUSE_ACC_DEEP
    (admitted past 256 columns and measured to pay) or 0.  The grad and the no-grad forward both ask here."""
    if fuse_acc_default(T, d_in, d_out, r, r_acc, kind, dtype, param_f32):
        return _lib.FUSE_ACC
    if deep_acc_admits(d_in, d_out, r, r_acc, kind, dtype, param_f32) and deep_acc_pays(T, d_in, d_out, r, r_acc):
        return _lib.FUSE_ACC_DEEP
    return 0


SHARED_FUSED_ACC_MIN_T = 8193          # more than 8192 tokens: the threshold of the streaming shared-input kernel
SHARED_FUSED_ACC_MAX_N = 4
SHARED_FUSED_ACC_MAX_LDS = 160 * 1024   # bytes of LDS a workgroup of chain_shared_acc.hip may plan


def shared_fused_acc_lds_bytes(r_tots: Sequence[int]) -> int:
    """The LDS plan of chain_shared_acc.hip for siblings of r_acc + r = r_tots: the H panels of every sibling (r_pad x 128
    bytes each, r_pad = ceil64(r_acc + r)) and the stage -- the widest sibling's packed-factor image with the 8 KiB input
    image in phase 1, at least 24 KiB (F2 panel groups, epilogue scratch) in phase 2."""
    r_pads = [(rt + 63) // 64 * 64 for rt in r_tots]
    return sum(rp * 128 for rp in r_pads) + max(max(r_pads) * 128 + 8192, 24576)


def shared_fused_acc_admits(T: int, d_in: int, layers: Sequence[Tuple[int, int, int, int]], dtype: torch.dtype,
                            param_f32: bool = False) -> bool:
    """The set sow_backward_shared admits under SOW_FUSE_ACC (include/sow_amd.h): `layers` = (d_out, r, r_acc, kind) of at
    most four siblings on one [T, d_in] input with T > 8192, EVERY one a low-rank-accumulator layer of the SOW_FUSE_ACC set
    (fused_acc_admits), whose LDS plan fits (three siblings of r_acc + r <= 256 always do, four of more than 192 do not).
    The call-time conditions (the flag in the dtype, 16-byte-aligned tensors, flagged workspaces, the NO_SHARED_X and
    NO_FUSED_ACC switches off) are not part of it."""
    if not 1 <= len(layers) <= SHARED_FUSED_ACC_MAX_N or T < SHARED_FUSED_ACC_MIN_T:
        return False
    if not all(fused_acc_admits(d_in, d_out, r, r_acc, kind, dtype, param_f32) for d_out, r, r_acc, kind in layers):
        return False
    return shared_fused_acc_lds_bytes([r + r_acc for _, r, r_acc, _ in layers]) <= SHARED_FUSED_ACC_MAX_LDS


SHARED_FUSED_ACC_PAYS_LDS = 80 * 1024   # the largest LDS plan at which two workgroups share a CU (160 KiB)


def shared_fused_acc_pays(r_tots: Sequence[int]) -> bool:
    """The measured dispatch rule of the module surface for the shared-input data gradient of low-rank-accumulator siblings
    (profiles/shared_fused_acc.txt): the sets whose LDS plan (shared_fused_acc_lds_bytes of the
    siblings' r_acc + r) leaves room for TWO workgroups per CU.

    Measured (bf16, T = 32768, r = 50; us per backward data pass, grouped path with the module surface's dX adds -> shared
    kernel, +- = spread of the window medians, LDS plan):
        q+k+v   3 x 512->512,  r_acc =  50 (r_pad 128,  72 KiB): 128.3 +- 7.0 ->  79.8   0.62   pays
        q+k+v   3 x 512->512,  r_acc = 100 (r_pad 192, 104 KiB): 141.6 +- 4.4 -> 159.0   1.12   loses
        q+k+v   3 x 512->512,  r_acc = 200 (r_pad 256, 136 KiB): 156.7 +- 6.8 -> 185.3   1.18   loses
        gate+up 2 x 512->1376, r_acc =  50 (r_pad 128,  56 KiB): 123.4 +- 6.3 ->  97.1   0.79   pays
        gate+up 2 x 512->1376, r_acc = 100 (r_pad 192,  80 KiB): 137.4 +- 8.9 -> 114.2   0.83   pays
        gate+up 2 x 512->1376, r_acc = 200 (r_pad 256, 104 KiB): 160.6 +- 5.7 -> 218.0   1.36   loses
    Every row at two workgroups per CU (plan <= 80 KiB) beats the grouped path by more than its spread; every row at one
    4-wave workgroup per CU loses to it: with nothing else resident the barriers of the 64-token tile code leave the CU idle.
    Those sets keep the grouped path.  NOT measured: r_pad = 64 sets (they plan at most 56 KiB: the paying class), f16, other
    widths."""
    return shared_fused_acc_lds_bytes(r_tots) <= SHARED_FUSED_ACC_PAYS_LDS


def acc_logical_shape(codes: torch.Tensor) -> Tuple[int, int]:
    """(d_in, d_out) of the matrix a codes tensor stands for (a format may pack several rows into one code element)."""
    fmt = BY_CODE_DTYPE.get(codes.dtype)
    return fmt.logical_shape(codes) if fmt else (codes.shape[0], codes.shape[1])


def acc_dequantize(codes: torch.Tensor, exps: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None):
    """The image W^ of a quantised accumulator (codes and their scales `exps`, of one format of acc_format.py), exactly, in bf16
    or f16 (the format's image entry, sow_acc_dequantize / sow_acc_dequantize_fp4: one streaming pass).  `out`: a [d_in, d_out]
    tensor of `dtype` whose rows are contiguous (any row pitch that is a multiple of 8), written in place."""
    dev = _need_gpu(codes, exps, out)
    fmt = BY_CODE_DTYPE.get(codes.dtype)
    if fmt is None or not fmt.well_formed(codes, exps):
        raise TypeError(f"sow_amd.acc_dequantize: {_NOT_A_PAIR}")
    if dtype not in _HALF:
        raise TypeError(f"sow_amd.acc_dequantize: the image is bfloat16 or float16, not {dtype}")
    d_in, d_out = fmt.logical_shape(codes)
    codes, exps = codes.contiguous(), exps.contiguous()
    if out is None:
        out = torch.empty((d_in, d_out), dtype=dtype, device=dev)
    elif out.dtype != dtype or tuple(out.shape) != (d_in, d_out) or (d_out > 1 and out.stride(1) != 1):
        raise ValueError("sow_amd.acc_dequantize: `out` must be a [d_in, d_out] tensor of the image dtype with contiguous rows")
    if d_in and d_out:
        _launch(dev, fmt.dequantize, getattr(_lib.load(), fmt.dequantize), _ptr(codes), _ptr(exps), d_in, d_out, _ptr(out),
                out.stride(0) if d_in > 1 else d_out, _DT[dtype])
    return out


# The scratch arena of the images: one buffer per (device, dtype), sized to the largest single call so far (one layer, or the
# siblings of a group), reused by every quantised layer in stream order.  An image is valid until the next acc_images() call
# for that (device, dtype) on the stream it was built on; nothing keeps it (autograd saves the codes and rebuilds it).
_ARENAS: dict = {}
_ARENAS_CAPTURED: set = set()    # arenas a HIP graph has recorded the address of ...
_ARENAS_RETIRED: list = []       # ... are kept alive when a larger one replaces them: a replay still writes there


def acc_images(pairs, dtype: torch.dtype) -> list:
    """The images of the E4M3 / MXFP4 accumulators `pairs` = [(codes, exps), ...] of ONE call, side by side in the scratch arena.
    The arena grows only outside graph capture: a capture needs one eager call of the same model first."""
    dev = pairs[0][0].device
    es = torch.empty((), dtype=dtype).element_size()
    shapes = [acc_logical_shape(c) for c, _ in pairs]
    sizes = [(a * b * es + 255) // 256 * 256 for a, b in shapes]
    need, key = sum(sizes), (dev, dtype)
    buf = _ARENAS.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if buf is None or buf.numel() < need:
        if capturing:
            raise RuntimeError("sow_amd: the scratch arena of the E4M3 accumulator images cannot grow during graph capture; "
                               "run the captured calls once eagerly first")
        if buf is not None and key in _ARENAS_CAPTURED:
            _ARENAS_RETIRED.append(buf)
            _ARENAS_CAPTURED.discard(key)
        with torch.cuda.device(dev):
            buf = _ARENAS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    if capturing:
        _ARENAS_CAPTURED.add(key)
    out, off = [], 0
    for (codes, exps), n, shape in zip(pairs, sizes, shapes):
        img = buf[off:off + shape[0] * shape[1] * es].view(dtype).view(shape)
        out.append(acc_dequantize(codes, exps, dtype, out=img))
        off += n
    return out


def acc_operands(accs, dtype: torch.dtype) -> list:
    """(acc_down, acc_up) of every layer of ONE call as the dense kernels read them: an E4M3 or MXFP4 accumulator (codes, exponents)
    is replaced by (its image in the scratch arena, None), everything else passes through."""
    quantised = [i for i, (d, _) in enumerate(accs) if d is not None and d.numel() and d.dtype in BY_CODE_DTYPE]
    if not quantised:
        return list(accs)
    out = list(accs)
    for i, img in zip(quantised, acc_images([accs[i] for i in quantised], dtype)):
        out[i] = (img, None)
    return out


def sow_forward(x2: torch.Tensor, A: torch.Tensor, B: torch.Tensor, acc_down, acc_up, bias, scale: float,
                save_h: bool = True, *, param_f32: bool = False, fuse_acc=False):
    """y, h_save = forward of the SoW contraction on a flattened [T, d_in] input.  save_h = False (no-grad / eval callers,
    e.g. the reload + generate loop of commonsense_evaluate.py:268-287): the projection is not written to HBM and None
    is returned in its place (every rank except r <= 64 with a dense accumulator, whose fused kernels write it as scratch;
    a wide layer off the fused chain keeps its intermediate in the forward workspace).
    param_f32: A, B and bias are fp32, x2 is bf16 / f16 (the compute dtype); the kernels round the
    parameters once to x2's dtype (include/sow_amd.h: SOW_PARAM_F32) and y is of x2's dtype.  The accumulator is fp32 too
    (rounded with them at every call) or of x2's dtype (native: read in place, SOW_ACC_NATIVE).
    fuse_acc: the call's permission (True or _lib.FUSE_ACC: SOW_FUSE_ACC; _lib.FUSE_ACC_DEEP: SOW_FUSE_ACC_DEEP) -- a low-rank
    accumulator and the live term in one pass where the library admits the call; the same result as without it everywhere
    else."""
    lib = _lib.load()
    dev = _need_gpu(x2, A, B, acc_down if acc_down is not None and acc_down.numel() else None,
                    acc_up if acc_up is not None and acc_up.numel() else None, bias)
    dt, pdt = _call_dtype(x2, param_f32, fuse_acc=fuse_acc, acc_down=acc_down)
    for name, t in (("A", A), ("B", B), ("bias", bias)):
        if t is not None and t.dtype != pdt:
            raise TypeError(f"sow_amd: dtype mismatch, x is {x2.dtype} but {name} is {t.dtype}"
                            + (" (parameters must be torch.float32)" if param_f32 else ""))
    T, d_in = x2.shape
    r, d_out = B.shape
    if A.shape != (d_in, r):
        raise ValueError(f"sow_amd: A has shape {tuple(A.shape)}, expected {(d_in, r)}")
    kind, r_acc = check_accumulator(x2, d_in, d_out, acc_down, acc_up, param_dtype=pdt if param_f32 else None)
    x2 = x2.contiguous()
    A, B = A.contiguous(), B.contiguous()
    acc_down = acc_down.contiguous() if kind != _lib.ACC_NONE else None
    acc_up = acc_up.contiguous() if kind == _lib.ACC_LOWRANK else None
    bias = bias.contiguous() if bias is not None else None
    y = torch.empty((T, d_out), dtype=x2.dtype, device=dev)
    h = None
    # a dense accumulator at r <= 64 takes the saved projection as scratch even when it is not kept: without it
    # sow_forward composes the product from two launches and rounds y twice (the training forward rounds it once)
    if save_h or (r <= 64 and kind == _lib.ACC_DENSE):
        h = torch.empty(T * (64 if r <= 64 else r), dtype=x2.dtype, device=dev)   # == sow_h_save_elems(T, r)
    # the forward touches a workspace only for some shapes (include/sow_amd.h: sow_forward_workspace_bytes)
    nws = _forward_workspace_bytes(lib, T, d_in, d_out, r, r_acc, kind, dt)
    ws = _ws(nws, dev) if nws else None
    _launch(dev, "sow_forward", lib.sow_forward, _ptr(x2), _ptr(A), _ptr(B), _ptr(acc_down), _ptr(acc_up), _ptr(bias), _ptr(y),
            _ptr(h), T, d_in, d_out, r, r_acc, kind, float(scale), dt, _ptr(ws), 0 if ws is None else ws.numel())
    return y, (h if save_h else None)


SKINNY_MAX_LAYERS = 16     # include/sow_amd.h: sow_forward_skinny admits at most 32 tokens per layer (SKINNY_MAX_T) and 16 layers per call
_SKINNY_WS_BYTES: dict = {}


def skinny_workspace_bytes(T: int, d_in: int, d_out: int, r: int, kind: int, dt: int) -> int:
    """sow_forward_skinny_workspace_bytes -- for a quantised accumulator the query of its format --, memoised per shape: 0 = the
    shape is outside the admitted set.  A pure function of the shape (no switch enters), so the memo is never dropped."""
    key = (T, d_in, d_out, r, kind, dt)
    n = _SKINNY_WS_BYTES.get(key)
    if n is None:
        lib, fmt = _lib.load(), BY_KIND.get(kind)
        n = _SKINNY_WS_BYTES[key] = int(lib.sow_forward_skinny_workspace_bytes(T, d_in, d_out, r, kind, dt) if fmt is None
                                        else getattr(lib, fmt.workspace_query)(T, d_in, d_out, r, dt))
    return n


_SKINNY_ROWS_WS_BYTES: dict = {}
_SKINNY_ROWS = SKINNY_MAX_T       # the most rows a no-grad module call sends to the skinny forward: sow_amd.skinny_rows / set_skinny_rows


def set_skinny_rows(n: int) -> int:
    """The most flattened rows (batch x beams of a decode step) at which no-grad SoWLinear / SiblingGroup calls take the fused
    skinny forward: 32 (the default: sow_forward_skinny alone) up to 64 (33 ... n rows go to sow_forward_skinny_rows).  Opt-in,
    because a call of 33 ... 64 rows then rounds y once from one fp32 sum where the default path rounds h B and the dense
    product as the training forward does: the results differ in the last bit.  Returns the value it replaces."""
    global _SKINNY_ROWS
    if isinstance(n, bool) or not isinstance(n, int) or not SKINNY_MAX_T <= n <= SKINNY_ROWS_MAX:
        raise ValueError(f"sow_amd.set_skinny_rows: {n!r} is not an int in [{SKINNY_MAX_T}, {SKINNY_ROWS_MAX}]")
    old, _SKINNY_ROWS = _SKINNY_ROWS, n
    return old


@contextlib.contextmanager
def skinny_rows(n: int):
    """with sow_amd.skinny_rows(64): ...  -- set_skinny_rows(n) for the block, the earlier value restored after it."""
    old = set_skinny_rows(n)
    try:
        yield
    finally:
        set_skinny_rows(old)


def skinny_rows_limit() -> int:
    return _SKINNY_ROWS


def skinny_rows_workspace_bytes(T: int, d_in: int, d_out: int, r: int, kind: int, dt: int) -> int:
    """sow_forward_skinny_rows_workspace_bytes (one query for every kind), memoised per shape: 0 = outside the admitted set."""
    key = (T, d_in, d_out, r, kind, dt)
    n = _SKINNY_ROWS_WS_BYTES.get(key)
    if n is None:
        n = _SKINNY_ROWS_WS_BYTES[key] = int(_lib.load().sow_forward_skinny_rows_workspace_bytes(T, d_in, d_out, r, kind, dt))
    return n


def skinny_rows_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule of the module surface at 33 ... 64 rows inside sow_amd.skinny_rows, for a bf16 / f16 dense
    accumulator or none (profiles/skinny_rows.txt; quantised formats: acc_format.py): the calls at which
    sow_forward_skinny_rows (n) is faster than sow_forward / sow_forward_group with a scratch h (a) by more than the larger
    run-to-run spread of the two.  Measured (us, bf16,
    r = 50, T = 33 / 64, n against a; +- the larger spread of the two): 4096->4096 38.0 / 43.2 against 234.6 / 129.7 (+- 2.7 / 2.1),
    4096->11008 64.7 / 73.6 against 378.0 / 130.2 (+- 1.0 / 0.9), 11008->4096 60.0 / 69.2 against 459.8 / 312.2 (+- 0.8 / 3.1),
    512->512 18.4 / 19.6 against 40.0 / 37.6 (+- 2.2 / 9.1), 512->1376 18.6 / 21.3 against 60.2 / 35.7 (+- 0.6 / 6.9), q + k + v of
    4096->4096 68.9 / 85.7 against 687.6 / 375.5 (+- 0.7 / 0.9); a / n lies between 1.68 and 9.98 in all 36 rows (T = 33, 48, 64;
    r = 8, 50) and the gap exceeds the spread in each: the rule excludes nothing.  n is also below two sow_forward_skinny calls on
    the row halves in every row (b2 / n 1.18 ... 1.94).  NOT measured: f16, widths above 11008."""
    return SKINNY_MAX_T < T <= SKINNY_ROWS_MAX


SHORT_ROWS_MAX = 1024      # include/sow_amd.h: SOW_SHORT_ROWS_MAX
_SHORT_ROWS = False        # sow_amd.short_rows / set_short_rows: training calls of short batches on the skinny kernel pair
_SHORT_WS_BYTES: dict = {}


def set_short_rows(on: bool) -> bool:
    """Whether bf16 / f16 dense-accumulator layers of at most 1024 flattened rows run forward and data gradient on the skinny
    kernel pair (sow_forward_short / sow_backward_short) where short_rows_pays admits the call.  Off by default: opt-in, because
    such a call rounds y and dX once from one fp32 sum where the default path's bits are pinned by the module tests.  Returns
    the value it replaces."""
    global _SHORT_ROWS
    if not isinstance(on, bool):
        raise ValueError(f"sow_amd.set_short_rows: {on!r} is not a bool")
    old, _SHORT_ROWS = _SHORT_ROWS, on
    return old


@contextlib.contextmanager
def short_rows(on: bool = True):
    """with sow_amd.short_rows(): ...  -- set_short_rows(on) for the block, the earlier value restored after it."""
    old = set_short_rows(on)
    try:
        yield
    finally:
        set_short_rows(old)


def short_rows_enabled() -> bool:
    return _SHORT_ROWS


def short_workspace_bytes(T: int, d_in: int, d_out: int, r: int, dt: int, forward_only: bool = False) -> int:
    """sow_short_workspace_bytes (forward_only: sow_forward_short_workspace_bytes) of a dense-accumulator layer, memoised per
    shape: 0 = outside the admitted set.  Pure functions of the shape."""
    key = (T, d_in, d_out, r, dt, forward_only)
    n = _SHORT_WS_BYTES.get(key)
    if n is None:
        lib = _lib.load()
        q = lib.sow_forward_short_workspace_bytes if forward_only else lib.sow_short_workspace_bytes
        n = _SHORT_WS_BYTES[key] = int(q(T, d_in, d_out, r, _lib.ACC_DENSE, dt))
    return n


# (d_in, d_out) -> the most rows at which the new pair won: the table of short_rows_pays' docstring
SHORT_ROWS_TABLE: dict = {(768, 768): 256, (768, 3072): 256, (3072, 768): 256, (4096, 4096): 128, (4096, 11008): 128,
                          (11008, 4096): 128, (512, 512): 256, (512, 1376): 256}


def short_rows_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule of the module surface inside sow_amd.short_rows (profiles/short_rows.txt, DESIGN.md section
    4.5e): the (rows, shape) classes at which forward + data gradient on sow_forward_short / sow_backward_short (n) beat
    sow_forward + the data phase of sow_backward_ex (a) by more than the larger run-to-run spread of the two.  One line per
    measured shape, the most rows up to which n won at EVERY measured row count and rank (bf16, MI355X):

        768->768: T <= 256
        768->3072: T <= 256
        3072->768: T <= 256
        4096->4096: T <= 128
        4096->11008: T <= 128
        11008->4096: T <= 128
        512->512: T <= 256
        512->1376: T <= 256

    Measured (us, forward + data gradient in one timed region, a against n, +- the larger spread): 768->768 r = 8 at T = 128 /
    256 / 512 / 1024: 68.3 / 69.0 / 69.3 / 70.8 against 37.9 / 44.7 / 73.1 / 121.1 (+- 2.5 / 2.3 / 2.6 / 2.0); 768->3072: 110.2 /
    109.0 / 91.5 / 90.4 against 53.6 / 76.4 / 120.5 / 219.7; 3072->768: 125.2 / 124.9 / 115.2 / 114.5 against 58.5 / 93.6 / 167.4
    / 303.3; 4096->4096 r = 50 at T = 65 / 128 / 256 / 512 / 1024: 205.5 / 203.5 / 203.9 / 137.3 / 138.5 against 106.0 / 145.3 /
    251.6 / 459.9 / 877.6; 4096->11008 r = 50: 298.3 / 300.0 / 252.8 / 212.9 / 224.1 against 194.8 / 258.0 / 475.2 / 921.0 /
    1845.3; 11008->4096 r = 50: 348.4 / 348.5 / 331.9 / 213.2 / 219.0 against 217.1 / 301.3 / 560.2 / 1085.4 / 2188.8; 512->512
    r = 50 at T = 256 / 1024: 64.7 / 66.1 against 41.6 / 97.3; 512->1376: 73.7 / 73.3 against 50.4 / 133.6.  n's time grows with
    the row blocks -- W is read once per 64 rows -- while a is flat and drops where its product leaves the generic GEMM, so a / n
    falls from 2.1 to 0.1 along every shape.
    The rule EXCLUDES: every row count above a shape's line (n lost there, or the count lies between a measured win and a
    measured loss: 257 ... 511 on the narrow shapes, 129 ... 255 on llama-7b's); every shape that was not measured; and calls
    of at most 64 rows, which the sweep does not hold.  NOT measured: f16, a full GLUE step, hardware counters."""
    tmax = SHORT_ROWS_TABLE.get((d_in, d_out), 0)
    return 64 < T <= tmax


def skinny_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule of the module surface (profiles/skinny_forward.txt): the token
    counts and widths at which the fused skinny forward is faster than the path it replaces (quantised formats: acc_format.py)."""
    return 1 <= T <= SKINNY_MAX_T


def skinny_acc(acc_down, acc_up):
    """The accumulator element of a sow_forward_skinny layer tuple: None, the dense tensor, or (codes, scales)."""
    if acc_down is None or acc_down.numel() == 0:
        return None
    return (acc_down, acc_up) if acc_down.dtype in BY_CODE_DTYPE else acc_down


def skinny_admits(x2: torch.Tensor, A: torch.Tensor, B: torch.Tensor, acc_down, acc_up, bias, mixed: bool = False) -> bool:
    """Whether a no-grad module call on the flattened input x2 may go to sow_forward_skinny: a bf16 / f16 call of at most 32
    tokens with parameters of the input's dtype -- or fp32 factors and bias (autocast with master factors: SOW_PARAM_F32 |
    SOW_ACC_NATIVE, the kernels round them in registers) --, a dense accumulator (in the input's dtype or as codes of a format)
    or none, and a shape the library admits and the dispatch rule keeps.  False sends the caller to the existing path, which
    raises whatever it raises today.  mixed: the call runs under autocast with fp32 factors and x2 already of the compute dtype."""
    dt = _DT.get(x2.dtype)
    if dt is None or dt == _lib.F32 or not x2.is_cuda or x2.dim() != 2 or not 1 <= x2.shape[0] <= _SKINNY_ROWS:
        return False
    rows = x2.shape[0] > SKINNY_MAX_T      # 33 ... sow_amd.skinny_rows: sow_forward_skinny_rows, its query and its rules
    kind, fmt = _acc_kind_fmt(acc_down, acc_up)
    if kind == _lib.ACC_LOWRANK or A.dim() != 2 or B.dim() != 2:
        return False
    T, d_in = x2.shape
    r, d_out = B.shape
    if tuple(A.shape) != (d_in, r) or (kind != _lib.ACC_NONE and tuple(acc_down.shape) != (
            d_in // fmt.rows_per_code if fmt else d_in, d_out)):     # (d_in is whole code rows: scales_fit asks for whole blocks below)
        return False
    pdt = torch.float32 if mixed else x2.dtype      # fp32 master factors (mixed: under autocast), or parameters of the input's dtype
    for t, want in ((A, pdt), (B, pdt), (bias, pdt), (acc_down if kind == _lib.ACC_DENSE else None, x2.dtype)):
        if t is not None and (t.dtype != want or t.device != x2.device):
            return False
    if pdt != x2.dtype:
        dt |= _lib.PARAM_F32 | _lib.ACC_NATIVE
    if fmt is not None and (acc_up is None or not fmt.scales_fit(acc_up, d_in, d_out) or acc_down.device != x2.device
                            or acc_up.device != x2.device or not (fmt.pays_rows if rows else fmt.pays)(T, d_in, d_out)):
        return False
    if rows:
        return skinny_rows_pays(T, d_in, d_out) and skinny_rows_workspace_bytes(T, d_in, d_out, r, kind, dt) > 0
    return skinny_pays(T, d_in, d_out) and skinny_workspace_bytes(T, d_in, d_out, r, kind, dt) > 0


def sow_forward_skinny_rows(layers) -> Optional[list]:
    """sow_forward_skinny for layers of up to 64 rows each (include/sow_amd.h: sow_forward_skinny_rows; layers of at most 32
    rows compute in it what they compute in sow_forward_skinny, bit for bit).  Same arguments, same result."""
    return _forward_skinny(layers, True)


def sow_forward_skinny(layers) -> Optional[list]:
    """y_i of n <= 16 independent generation-sized layer calls (T_i <= 32 tokens) in two launches (include/sow_amd.h:
    sow_forward_skinny).  `layers`: one (x2, A, B, acc_down, bias, scale) per layer -- x2 [T, d_in] bf16 / f16, acc_down the
    dense accumulator, the (codes, scales) pair of a quantised one (TypeError unless well formed: acc_format.py), or None.  A, B and bias are of x2's dtype, or fp32 in every
    layer of the call (SOW_PARAM_F32 | SOW_ACC_NATIVE: rounded once in registers, the accumulator stays of x2's dtype).  Returns the list of outputs, or None when the library refuses the set (nothing was launched:
    the caller runs sow_forward / LayerGroup instead)."""
    return _forward_skinny(layers, False)


def _forward_skinny(layers, _rows: bool) -> Optional[list]:
    """sow_forward_skinny (_rows: sow_forward_skinny_rows): the one body of both."""
    lib = _lib.load()
    name = "sow_amd.sow_forward_skinny_rows" if _rows else "sow_amd.sow_forward_skinny"
    n = len(layers)
    if n == 0:
        return []
    if n > SKINNY_MAX_LAYERS:
        return None
    x0 = layers[0][0]
    dt = _dt(x0)
    pdt = x0.dtype
    if layers[0][1].dtype == torch.float32 and dt != _lib.F32:      # fp32 master factors over a native accumulator
        pdt, dt = torch.float32, dt | _lib.PARAM_F32 | _lib.ACC_NATIVE
    keep, sizes, total = [], [], 0
    for x2, A, B, acc_down, bias, scale in layers:
        exps = fmt = None
        if isinstance(acc_down, tuple):
            acc_down, exps = acc_down
            fmt = BY_CODE_DTYPE.get(acc_down.dtype)
            if fmt is None or not fmt.well_formed(acc_down, exps):
                raise TypeError(f"{name}: {_NOT_A_PAIR}")
        dev = _need_gpu(x2, A, B, acc_down, exps, bias)
        if dev != x0.device or any(t is not None and t.dtype != x0.dtype for t in (x2, acc_down if exps is None else None)) or any(
                t is not None and t.dtype != pdt for t in (A, B, bias)):
            raise TypeError(f"{name}: the inputs and dense accumulators of a call share one dtype, its factors "
                            "and biases one dtype (the inputs', or float32), and all tensors one device")
        T, d_in = x2.shape
        r, d_out = B.shape
        if tuple(A.shape) != (d_in, r) or (acc_down is not None and (fmt.logical_shape(acc_down) if fmt else tuple(acc_down.shape[:2])) != (d_in, d_out)) or (
                bias is not None and tuple(bias.shape) != (d_out,)):
            raise ValueError(f"{name}: operand shapes do not match")
        kind = _lib.ACC_NONE if acc_down is None else _lib.ACC_DENSE if fmt is None else fmt.kind
        nws = (skinny_rows_workspace_bytes if _rows else skinny_workspace_bytes)(T, d_in, d_out, r, kind, dt) if T else 0
        if T and not nws:
            return None
        nws = (nws + 255) & ~255
        keep.append((x2.contiguous(), A.contiguous(), B.contiguous(), None if acc_down is None else acc_down.contiguous(),
                     None if bias is None else bias.contiguous(), None if exps is None else exps.contiguous(), kind))
        sizes.append((total, nws))
        total += nws
    ws = _ws(total, x0.device)       # one allocation, carved at 256-byte offsets
    base = ws.data_ptr()
    arr = (_lib.LayerArgs * n)()
    ys = []
    for i, ((x2, A, B, acc_down, bias, exps, kind), (off, nws), layer) in enumerate(zip(keep, sizes, layers)):
        y = torch.empty((x2.shape[0], B.shape[1]), dtype=x2.dtype, device=x0.device)
        ys.append(y)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.bias, a.y = _ptr(x2), _ptr(A), _ptr(B), _ptr(acc_down), _ptr(bias), _ptr(y)
        a.T, a.d_in, a.d_out, a.r_live = x2.shape[0], x2.shape[1], B.shape[1], B.shape[0]
        a.acc_up, a.acc_kind = _ptr(exps), kind
        a.scale = float(layer[5])
        a.workspace, a.workspace_bytes = base + off, nws
    rc = _launch_rc(x0.device, lib.sow_forward_skinny_rows if _rows else lib.sow_forward_skinny, arr, n, dt)
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "sow_forward_skinny_rows" if _rows else "sow_forward_skinny")
    return ys


def short_admits(x2: torch.Tensor, A: torch.Tensor, B: torch.Tensor, acc_down, acc_up, bias) -> bool:
    """Whether a module call on the flattened input x2 goes to sow_forward_short / sow_backward_short: inside sow_amd.short_rows,
    a bf16 / f16 call with parameters of the input's dtype, a dense accumulator of that dtype (the image of a quantised one
    included: pass the image), a shape the library admits and short_rows_pays keeps.  False keeps the existing path."""
    if not _SHORT_ROWS:
        return False
    dt = _DT.get(x2.dtype)
    if dt is None or dt == _lib.F32 or not x2.is_cuda or x2.dim() != 2 or A.dim() != 2 or B.dim() != 2:
        return False
    if acc_down is None or acc_down.numel() == 0 or acc_down.dtype in BY_CODE_DTYPE or (acc_up is not None and acc_up.numel()):
        return False
    T, d_in = x2.shape
    r, d_out = B.shape
    if tuple(A.shape) != (d_in, r) or tuple(acc_down.shape) != (d_in, d_out) or (bias is not None and tuple(bias.shape) != (d_out,)):
        return False
    for t in (A, B, bias, acc_down):
        if t is not None and (t.dtype != x2.dtype or t.device != x2.device):
            return False
    return short_rows_pays(T, d_in, d_out) and short_workspace_bytes(T, d_in, d_out, r, dt) > 0


def _short_args(n: int):
    return (_lib.LayerArgs * n)()


def sow_forward_short(layers, save_h: bool = True):
    """(ys, hs) of n <= 16 dense-accumulator layer calls of at most 1024 rows each through sow_forward_short (include/sow_amd.h):
    `layers` = one (x2, A, B, acc_down, bias, scale) per layer, everything of x2's dtype.  hs[i] is the h_save the weight phases
    read, or None with save_h = False (a no-grad call).  None when the library refuses the set: nothing was launched."""
    lib = _lib.load()
    n = len(layers)
    if n == 0:
        return [], []
    if n > SKINNY_MAX_LAYERS:
        return None
    x0 = layers[0][0]
    dt = _dt(x0)
    keep, sizes, total = [], [], 0
    for x2, A, B, acc_down, bias, scale in layers:
        dev = _need_gpu(x2, A, B, acc_down, bias)
        if dev != x0.device or any(t is not None and t.dtype != x0.dtype for t in (x2, A, B, acc_down, bias)):
            raise TypeError("sow_amd.sow_forward_short: the tensors of a call share one dtype and one device")
        T, d_in = x2.shape
        r, d_out = B.shape
        if tuple(A.shape) != (d_in, r) or tuple(acc_down.shape) != (d_in, d_out) or (bias is not None and tuple(bias.shape) != (d_out,)):
            raise ValueError("sow_amd.sow_forward_short: operand shapes do not match")
        nws = short_workspace_bytes(T, d_in, d_out, r, dt, forward_only=True) if T else 0
        if T and not nws:
            return None
        nws = (nws + 255) & ~255
        keep.append((x2.contiguous(), A.contiguous(), B.contiguous(), acc_down.contiguous(), None if bias is None else bias.contiguous()))
        sizes.append((total, nws))
        total += nws
    ws = _ws(total, x0.device)
    base = ws.data_ptr()
    arr = _short_args(n)
    ys, hs = [], []
    for i, ((x2, A, B, acc_down, bias), (off, nws), layer) in enumerate(zip(keep, sizes, layers)):
        T, d_out = x2.shape[0], B.shape[1]
        y = torch.empty((T, d_out), dtype=x2.dtype, device=x0.device)
        h = torch.empty(T * 64, dtype=x2.dtype, device=x0.device) if save_h else None
        ys.append(y)
        hs.append(h)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.bias, a.y, a.h_save = _ptr(x2), _ptr(A), _ptr(B), _ptr(acc_down), _ptr(bias), _ptr(y), _ptr(h)
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, x2.shape[1], d_out, B.shape[0], _lib.ACC_DENSE, float(layer[5])
        a.workspace, a.workspace_bytes = base + off, nws
    rc = _launch_rc(x0.device, lib.sow_forward_short, arr, n, dt)
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "sow_forward_short")
    return ys, hs


def sow_backward_short(layers):
    """[(dx, dA, dB, dbias)] of n <= 16 layer calls: the data gradients through sow_backward_short (one call for the set), then the
    existing weight phases of every layer on the same workspace (sow_backward with SOW_BWD_WEIGHTS), which read the dh the data
    phase left there.  `layers` = one (dy2, x2, h, A, B, acc_down, scale, need_bias) per layer, h from sow_forward_short."""
    lib = _lib.load()
    n = len(layers)
    if n == 0:
        return []
    x0 = layers[0][1]
    dt = _dt(x0)
    arr = _short_args(n)
    keep = []
    for i, (dy2, x2, h, A, B, acc_down, scale, need_bias) in enumerate(layers):
        dev = _need_gpu(dy2, x2, h, A, B, acc_down)
        if any(t.dtype != x0.dtype or t.device != x0.device for t in (dy2, x2, h, A, B, acc_down)):
            raise TypeError("sow_amd.sow_backward_short: the tensors of a call share one dtype and one device")
        T, d_in = x2.shape
        r, d_out = B.shape
        dy2, A, B, acc_down = dy2.contiguous(), A.contiguous(), B.contiguous(), acc_down.contiguous()
        nws = short_workspace_bytes(T, d_in, d_out, r, dt)
        if T and not nws:
            raise ValueError("sow_amd.sow_backward_short: the library does not admit this layer")
        ws = _ws(nws, dev)
        dx = torch.empty((T, d_in), dtype=x2.dtype, device=dev)
        a = arr[i]
        a.dy, a.dx, a.A, a.B, a.acc_down = _ptr(dy2), _ptr(dx), _ptr(A), _ptr(B), _ptr(acc_down)
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, _lib.ACC_DENSE, float(scale)
        a.workspace, a.workspace_bytes = _ptr(ws), ws.numel()
        keep.append((dy2, A, B, acc_down, ws, dx))
    _launch(x0.device, "sow_backward_short", lib.sow_backward_short, arr, n, dt)
    out = []
    for (dy2, A, B, acc_down, ws, dx), (_, x2, h, _, _, _, scale, need_bias) in zip(keep, layers):
        if x2.shape[0] == 0:
            out.append(sow_backward(dy2, x2, h, A, B, acc_down, None, scale, need_bias))
        else:
            out.append(sow_backward(dy2, x2, h, A, B, acc_down, None, scale, need_bias, phases=_lib.BWD_WEIGHTS, dx=dx, workspace=ws))
    return out


_SHORT_CODES = False       # sow_amd.short_codes / set_short_codes: inside short_rows, quantised layers read their codes in place
_SHORT_CODES_WS_BYTES: dict = {}


def set_short_codes(on: bool) -> bool:
    """Whether, INSIDE sow_amd.short_rows, a layer whose dense accumulator is quantised (E4M3 / MXFP4) runs forward and data gradient
    on the codes read in place (sow_forward_short_codes / sow_backward_short_codes: no image pass, no arena traffic) where the
    format's pays_short rule admits the call.  Off by default and inert outside short_rows: with it off, a quantised layer inside
    short_rows does what it did before (the image, then short_rows_pays).  Returns the value it replaces."""
    global _SHORT_CODES
    if not isinstance(on, bool):
        raise ValueError(f"sow_amd.set_short_codes: {on!r} is not a bool")
    old, _SHORT_CODES = _SHORT_CODES, on
    return old


@contextlib.contextmanager
def short_codes(on: bool = True):
    """with sow_amd.short_rows(), sow_amd.short_codes(): ...  -- set_short_codes(on) for the block, the earlier value restored after it."""
    old = set_short_codes(on)
    try:
        yield
    finally:
        set_short_codes(old)


def short_codes_enabled() -> bool:
    """The switch itself; it routes calls only while short_rows_enabled() holds too (short_codes_admits)."""
    return _SHORT_CODES


def short_codes_workspace_bytes(T: int, d_in: int, d_out: int, r: int, kind: int, dt: int, forward_only: bool = False) -> int:
    """sow_short_codes_workspace_bytes (forward_only: sow_forward_short_codes_workspace_bytes), memoised per shape: 0 = outside the
    admitted set.  Pure functions of the shape."""
    key = (T, d_in, d_out, r, kind, dt, forward_only)
    n = _SHORT_CODES_WS_BYTES.get(key)
    if n is None:
        lib = _lib.load()
        q = lib.sow_forward_short_codes_workspace_bytes if forward_only else lib.sow_short_codes_workspace_bytes
        n = _SHORT_CODES_WS_BYTES[key] = int(q(T, d_in, d_out, r, kind, dt))
    return n


def short_codes_admits(x2: torch.Tensor, A: torch.Tensor, B: torch.Tensor, acc_down, acc_up, bias) -> bool:
    """Whether a module call on the flattened input x2 goes to sow_forward_short_codes / sow_backward_short_codes: inside
    sow_amd.short_rows AND sow_amd.short_codes, a bf16 / f16 call with parameters of the input's dtype, a well-formed (codes,
    scales) pair of a format, a shape the library admits and the format's pays_short keeps.  False keeps the existing path."""
    if not (_SHORT_ROWS and _SHORT_CODES):
        return False
    dt = _DT.get(x2.dtype)
    if dt is None or dt == _lib.F32 or not x2.is_cuda or x2.dim() != 2 or A.dim() != 2 or B.dim() != 2:
        return False
    fmt = BY_CODE_DTYPE.get(acc_down.dtype) if acc_down is not None and acc_down.numel() else None
    if fmt is None or acc_up is None or not fmt.well_formed(acc_down, acc_up):
        return False
    T, d_in = x2.shape
    r, d_out = B.shape
    if tuple(A.shape) != (d_in, r) or fmt.logical_shape(acc_down) != (d_in, d_out) or (bias is not None and tuple(bias.shape) != (d_out,)):
        return False
    if any(t is not None and (t.dtype != x2.dtype or t.device != x2.device) for t in (A, B, bias)) or any(
            t.device != x2.device for t in (acc_down, acc_up)):
        return False
    return fmt.pays_short(T, d_in, d_out) and short_codes_workspace_bytes(T, d_in, d_out, r, fmt.kind, dt) > 0


def _codes_pair(acc, name: str):
    """(codes, scales, format) of the accumulator element of a sow_*_short_codes layer tuple."""
    if not isinstance(acc, tuple) or len(acc) != 2:
        raise TypeError(f"{name}: {_NOT_A_PAIR}")
    codes, scales = acc
    fmt = BY_CODE_DTYPE.get(codes.dtype)
    if fmt is None or not fmt.well_formed(codes, scales):
        raise TypeError(f"{name}: {_NOT_A_PAIR}")
    return codes.contiguous(), scales.contiguous(), fmt


def sow_forward_short_codes(layers, save_h: bool = True):
    """sow_forward_short on codes read in place (include/sow_amd.h: sow_forward_short_codes): `layers` = one (x2, A, B, (codes,
    scales), bias, scale) per layer, all pairs of ONE format, everything else of x2's dtype.  Returns (ys, hs) as sow_forward_short,
    None when the library refuses the set: nothing was launched.  No image is built and the arena is not touched."""
    lib = _lib.load()
    name = "sow_amd.sow_forward_short_codes"
    n = len(layers)
    if n == 0:
        return [], []
    if n > SKINNY_MAX_LAYERS:
        return None
    x0 = layers[0][0]
    dt = _dt(x0)
    keep, sizes, total = [], [], 0
    for x2, A, B, acc, bias, scale in layers:
        codes, scales, fmt = _codes_pair(acc, name)
        dev = _need_gpu(x2, A, B, codes, scales, bias)
        if dev != x0.device or any(t is not None and t.dtype != x0.dtype for t in (x2, A, B, bias)):
            raise TypeError(f"{name}: the tensors of a call share one dtype and one device")
        T, d_in = x2.shape
        r, d_out = B.shape
        if tuple(A.shape) != (d_in, r) or fmt.logical_shape(codes) != (d_in, d_out) or (bias is not None and tuple(bias.shape) != (d_out,)):
            raise ValueError(f"{name}: operand shapes do not match")
        nws = short_codes_workspace_bytes(T, d_in, d_out, r, fmt.kind, dt, forward_only=True) if T else 0
        if T and not nws:
            return None
        nws = (nws + 255) & ~255
        keep.append((x2.contiguous(), A.contiguous(), B.contiguous(), codes, scales, None if bias is None else bias.contiguous(), fmt.kind))
        sizes.append((total, nws))
        total += nws
    ws = _ws(total, x0.device)
    base = ws.data_ptr()
    arr = _short_args(n)
    ys, hs = [], []
    for i, ((x2, A, B, codes, scales, bias, kind), (off, nws), layer) in enumerate(zip(keep, sizes, layers)):
        T, d_out = x2.shape[0], B.shape[1]
        y = torch.empty((T, d_out), dtype=x2.dtype, device=x0.device)
        h = torch.empty(T * 64, dtype=x2.dtype, device=x0.device) if save_h else None
        ys.append(y)
        hs.append(h)
        a = arr[i]
        a.x, a.A, a.B, a.acc_down, a.acc_up, a.bias, a.y, a.h_save = (_ptr(x2), _ptr(A), _ptr(B), _ptr(codes), _ptr(scales), _ptr(bias),
                                                                      _ptr(y), _ptr(h))
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, x2.shape[1], d_out, B.shape[0], kind, float(layer[5])
        a.workspace, a.workspace_bytes = base + off, nws
    rc = _launch_rc(x0.device, lib.sow_forward_short_codes, arr, n, dt)
    if rc == _lib.ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "sow_forward_short_codes")
    return ys, hs


def sow_backward_short_codes(layers):
    """[(dx, dA, dB, dbias)] of n <= 16 layer calls: the data gradients through sow_backward_short_codes on the codes (one call for
    the set), then the existing weight phases of every layer on the same workspace.  The weight phases read x, h, dY and dh and no
    accumulator: they are called with kind SOW_ACC_DENSE (the plan the workspace is sized for) and the codes' address in acc_down's
    place, which is checked against NULL and never read.  `layers` = one (dy2, x2, h, A, B, (codes, scales), scale, need_bias) per
    layer, h from sow_forward_short_codes."""
    lib = _lib.load()
    name = "sow_amd.sow_backward_short_codes"
    n = len(layers)
    if n == 0:
        return []
    x0 = layers[0][1]
    dt = _dt(x0)
    arr = _short_args(n)
    keep = []
    for i, (dy2, x2, h, A, B, acc, scale, need_bias) in enumerate(layers):
        codes, scales, fmt = _codes_pair(acc, name)
        dev = _need_gpu(dy2, x2, h, A, B, codes, scales)
        if any(t.dtype != x0.dtype or t.device != x0.device for t in (dy2, x2, h, A, B)):
            raise TypeError(f"{name}: the tensors of a call share one dtype and one device")
        T, d_in = x2.shape
        r, d_out = B.shape
        dy2, x2, A, B = dy2.contiguous(), x2.contiguous(), A.contiguous(), B.contiguous()
        nws = short_codes_workspace_bytes(T, d_in, d_out, r, fmt.kind, dt) if T else 0
        if T and not nws:
            raise ValueError(f"{name}: the library does not admit this layer")
        ws = _ws(max(nws, 256), dev)
        dx = torch.empty((T, d_in), dtype=x2.dtype, device=dev)
        a = arr[i]
        a.dy, a.dx, a.A, a.B, a.acc_down, a.acc_up = _ptr(dy2), _ptr(dx), _ptr(A), _ptr(B), _ptr(codes), _ptr(scales)
        a.T, a.d_in, a.d_out, a.r_live, a.acc_kind, a.scale = T, d_in, d_out, r, fmt.kind, float(scale)
        a.workspace, a.workspace_bytes = _ptr(ws), ws.numel()
        keep.append((dy2, x2, A, B, codes, scales, ws, dx))
    _launch(x0.device, "sow_backward_short_codes", lib.sow_backward_short_codes, arr, n, dt)
    out = []
    for (dy2, x2, A, B, codes, scales, ws, dx), (_, _, h, _, _, _, scale, need_bias) in zip(keep, layers):
        T, d_in = x2.shape
        r, d_out = B.shape
        dA = torch.empty((d_in, r), dtype=x2.dtype, device=x2.device)
        dB = torch.empty((r, d_out), dtype=x2.dtype, device=x2.device)
        dbias = torch.empty((d_out,), dtype=x2.dtype, device=x2.device) if need_bias else None
        _launch(x2.device, "sow_backward", lib.sow_backward_ex, _ptr(dy2), _ptr(x2), _ptr(h), _ptr(A), _ptr(B), _ptr(codes), None,
                _ptr(dx), _ptr(dA), _ptr(dB), _ptr(dbias), T, d_in, d_out, r, 0, _lib.ACC_DENSE, float(scale), 0.0, dt,
                _ptr(ws), ws.numel(), int(_lib.BWD_WEIGHTS))
        out.append((dx, dA, dB, dbias))
    return out


def workspace_bytes(T: int, d_in: int, d_out: int, r: int, r_acc: int, kind: int, dtype: torch.dtype,
                    param_f32: bool = False, fuse_acc=False, native: bool = False) -> int:
    """native: the accumulator next to fp32 parameters is of the compute dtype (acc_native): no room for its packed copy."""
    flags = (_lib.PARAM_F32 | (_lib.ACC_NATIVE if native and kind != _lib.ACC_NONE else 0) if param_f32
             else (_perm(fuse_acc) if dtype != torch.float32 else 0))
    return _workspace_bytes(_lib.load(), T, d_in, d_out, r, r_acc, kind, _DT[dtype] | flags)


def sow_backward(dy2: torch.Tensor, x2: torch.Tensor, h: torch.Tensor, A: torch.Tensor, B: torch.Tensor, acc_down,
                 acc_up, scale: float, need_bias: bool,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = None,
                 grad_beta: float = 0.0, *, phases: int = _lib.BWD_DATA | _lib.BWD_WEIGHTS,
                 dx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, param_f32: bool = False,
                 fuse_acc=False):
    """dx, dA, dB, dbias.  `out` = (dA, dB, dbias) buffers to write/accumulate into (grad_beta).
    `phases` selects the data-gradient and / or weight-gradient kernels (see include/sow_amd.h); a split
    call must pass the same `workspace` (and `dx`) to both phases, each enqueued on the current stream.
    param_f32: fp32 parameters with bf16 / f16 activations (sow_forward); dA, dB and dbias are then fp32, dx of x2's dtype.
    fuse_acc: the permission for the data gradient (sow_forward); a workspace passed in must then come from
    workspace_bytes(..., fuse_acc=the same value), a smaller one makes the call run the unflagged kernels."""
    lib = _lib.load()
    dev = _need_gpu(dy2, x2, h, A, B)
    dt, pdt = _call_dtype(x2, param_f32, fuse_acc=fuse_acc, acc_down=acc_down)
    if dy2.dtype != x2.dtype:
        raise TypeError(f"sow_amd: grad dtype {dy2.dtype} differs from input dtype {x2.dtype}")
    if param_f32 and (A.dtype != pdt or B.dtype != pdt):
        raise TypeError("sow_amd: param_f32 needs torch.float32 factors")
    T, d_in = x2.shape
    r, d_out = B.shape
    kind = acc_kind(acc_down, acc_up)
    r_acc = acc_down.shape[1] if kind == _lib.ACC_LOWRANK else 0
    dy2 = dy2.contiguous()
    if dx is None:
        dx = torch.empty((T, d_in), dtype=x2.dtype, device=dev)
    if out is None:
        dA = torch.empty((d_in, r), dtype=pdt, device=dev)
        dB = torch.empty((r, d_out), dtype=pdt, device=dev)
        dbias = torch.empty((d_out,), dtype=pdt, device=dev) if need_bias else None
        grad_beta = 0.0
    else:
        dA, dB, dbias = out
        if any(g is not None and g.dtype != pdt for g in out):
            raise TypeError(f"sow_amd: gradient buffers must be {pdt}")
    nws = _workspace_bytes(lib, T, d_in, d_out, r, r_acc, kind, dt)
    ws = _ws(nws, dev) if workspace is None else workspace
    if ws.numel() < nws and dt & _PERMS:   # a permission: a workspace of the unflagged plan runs the unflagged kernels
        nws = _workspace_bytes(lib, T, d_in, d_out, r, r_acc, kind, dt & ~_PERMS)
    if ws.numel() < nws:
        raise ValueError("sow_amd: workspace too small")
    _launch(dev, "sow_backward", lib.sow_backward_ex, _ptr(dy2), _ptr(x2), _ptr(h), _ptr(A), _ptr(B),
            _ptr(acc_down) if kind != _lib.ACC_NONE else None, _ptr(acc_up) if kind == _lib.ACC_LOWRANK else None,
            _ptr(dx), _ptr(dA), _ptr(dB), _ptr(dbias), T, d_in, d_out, r, r_acc, kind, float(scale), float(grad_beta), dt,
            _ptr(ws), ws.numel(), int(phases))
    return dx, dA, dB, dbias


class LayerCall:
    """Arguments of one SoWLinear forward / backward inside a grouped call (include/sow_amd.h: sow_layer_args).  Static
    training buffers: build once, reuse every step.  `out` = (dA, dB, dbias) gradient buffers, `workspace` this layer's
    own workspace (workspace_bytes())."""

    def __init__(self, x2, A, B, *, acc_down=None, acc_up=None, bias=None, scale=1.0, y=None, h=None, dy2=None, dx=None,
                 out=None, grad_beta=0.0, workspace=None, forward_only=False, save_h=True, param_f32=False, fuse_acc=False):
        dev = _need_gpu(x2, A, B, bias, y, h, dy2, dx, workspace)
        # param_f32: fp32 A, B, bias, accumulator and gradients, activations of the compute dtype (SOW_PARAM_F32)
        # fuse_acc: the call's permission (_perm); it rides in the dtype, so the workspace queries below are the flagged ones
        self.dtype, pdt = _call_dtype(x2, param_f32, "sow_amd.LayerCall", fuse_acc=fuse_acc, acc_down=acc_down)
        adt = x2.dtype if self.dtype & _lib.ACC_NATIVE else pdt      # a native accumulator is of the compute dtype
        T, d_in = x2.shape
        r, d_out = B.shape
        # the same accumulator checks as the single-layer entry point (ops.sow_forward): same exceptions for the same input
        kind, _ = check_accumulator(x2, d_in, d_out, acc_down, acc_up, "sow_amd.LayerCall", param_dtype=pdt if param_f32 else None)
        for name, t, want in (("x", x2, x2.dtype), ("A", A, pdt), ("B", B, pdt), ("bias", bias, pdt), ("y", y, x2.dtype),
                              ("dy", dy2, x2.dtype), ("dx", dx, x2.dtype),
                              ("acc_down", acc_down if kind != _lib.ACC_NONE else None, adt),
                              ("acc_up", acc_up if kind == _lib.ACC_LOWRANK else None, adt)):
            if t is not None and (not t.is_contiguous() or t.dtype != want):
                raise ValueError(f"sow_amd.LayerCall: {name} must be contiguous and of the "
                                 + ("input" if want == x2.dtype else "parameter") + " dtype")
        if A.shape != (d_in, r):
            raise ValueError("sow_amd.LayerCall: factor shapes do not match the input")
        self.device, self.kind = dev, kind
        self.legacy_acc = bool(param_f32) and kind != _lib.ACC_NONE and not self.dtype & _lib.ACC_NATIVE   # an fp32 accumulator
        self.y = y if y is not None else torch.empty((T, d_out), dtype=x2.dtype, device=dev)
        # save_h = False (forward_only calls that no backward follows): h_save = NULL, the projection stays on chip --
        # except with a dense accumulator, whose single-launch kernels need the buffer (as in sow_forward)
        self.h = h if h is not None else (torch.empty(T * (64 if r <= 64 else r), dtype=x2.dtype, device=dev)
                                          if (save_h or not forward_only or (r <= 64 and kind == _lib.ACC_DENSE)) else None)
        self.dx = dx
        r_acc = acc_down.shape[1] if kind == _lib.ACC_LOWRANK else 0
        # a forward-only call needs scratch for a few shapes only (sow_forward_workspace_bytes), often none at all
        nws = (_forward_workspace_bytes(_lib.load(), T, d_in, d_out, r, r_acc, kind, self.dtype) if forward_only
               else _workspace_bytes(_lib.load(), T, d_in, d_out, r, r_acc, kind, self.dtype))
        self.workspace = workspace if workspace is not None else (_ws(nws, dev) if nws else None)
        if self.workspace is not None and self.workspace.numel() < nws and self.dtype & _PERMS:
            # a permission: a caller's workspace of the unflagged plan runs the two-pass kernels
            q = _forward_workspace_bytes if forward_only else _workspace_bytes
            nws = q(_lib.load(), T, d_in, d_out, r, r_acc, kind, self.dtype & ~_PERMS)
        if self.workspace is not None and self.workspace.numel() < nws:
            raise ValueError("sow_amd.LayerCall: workspace too small")
        dA, dB, dbias = out if out is not None else (None, None, None)
        # the kernels write gradients of the parameter dtype (fp32 under param_f32): a buffer of another dtype or shape
        # would be written out of bounds
        for name, g, shape in (("dA", dA, (d_in, r)), ("dB", dB, (r, d_out)), ("dbias", dbias, (d_out,))):
            if g is not None and (not g.is_contiguous() or g.dtype != pdt or tuple(g.shape) != shape or g.device != dev):
                raise ValueError(f"sow_amd.LayerCall: gradient buffer {name} must be a contiguous {pdt} tensor of shape "
                                 f"{shape} on {dev}")
        self._keep = (x2, A, B, acc_down, acc_up, bias, dy2, dA, dB, dbias)     # the struct holds raw pointers
        self.args = _lib.LayerArgs(
            x=_ptr(x2), A=_ptr(A), B=_ptr(B), acc_down=_ptr(acc_down) if kind != _lib.ACC_NONE else None,
            acc_up=_ptr(acc_up) if kind == _lib.ACC_LOWRANK else None, bias=_ptr(bias), y=_ptr(self.y), h_save=_ptr(self.h),
            dy=_ptr(dy2), dx=_ptr(dx), dA=_ptr(dA), dB=_ptr(dB), dbias=_ptr(dbias), T=T, d_in=d_in, d_out=d_out, r_live=r,
            r_acc=acc_down.shape[1] if kind == _lib.ACC_LOWRANK else 0, acc_kind=kind, scale=float(scale),
            grad_beta=float(grad_beta), workspace=_ptr(self.workspace),
            workspace_bytes=0 if self.workspace is None else self.workspace.numel())


class LayerGroup:
    """n independent layer calls issued through sow_forward_group / sow_backward_group: layers on the bf16 / f16 streaming
    kernels share launches (q / k / v; gate / up).  Outputs, input gradients and saved projections are bit-identical to n
    single calls; the weight gradients of a group large enough for the row-owner kernel (a whole decoder block) are summed
    over differently cut token slabs and agree to fp32 rounding of those sums.  bf16 takes the row-owner kernel under the
    default phases too; f16 takes it only when `phases` carries BWD_GROUP_SLABS (the deferred reduction of FactorBucket),
    so that backward() of an f16 group with the default phases stays bit-identical to single calls."""

    def __init__(self, calls: Sequence[LayerCall]):
        if not calls:
            raise ValueError("empty group")
        if len({c.dtype & ~(_PERMS | _lib.ACC_NATIVE) for c in calls}) != 1 or len({c.device for c in calls}) != 1:
            raise ValueError("sow_amd.LayerGroup: all layers must share dtype and device")
        # SOW_ACC_NATIVE rides in the dtype of the whole C call: layers without accumulator go with either form, but a native
        # accumulator and an fp32 one cannot share a call
        native = _lib.ACC_NATIVE if any(c.dtype & _lib.ACC_NATIVE for c in calls) else 0
        if native and any(c.legacy_acc for c in calls):
            raise ValueError("sow_amd.LayerGroup: fp32 parameters -- the accumulators of one group are all fp32 or all of the "
                             "compute dtype")
        self.calls = list(calls)
        self.arr = (_lib.LayerArgs * len(calls))(*[c.args for c in calls])
        # A permission rides in the dtype of the whole C call and belongs to each LayerCall: a group whose layers hold
        # different values (none, SOW_FUSE_ACC, SOW_FUSE_ACC_DEEP) issues its forward and its data gradient as one C call
        # per value (such layers never share a launch anyway: a low-rank accumulator takes the per-layer fall-through).  The
        # weight-gradient phases and their plans ignore the flags and always see the whole group.
        self._perms = [c.dtype & _PERMS for c in calls]
        mixed = len(set(self._perms)) > 1
        self._fused = [p == _lib.FUSE_ACC for p in self._perms] if mixed else None   # None: one value, one C call
        self.dtype = calls[0].dtype & ~(_PERMS | _lib.ACC_NATIVE) | native | (0 if mixed else self._perms[0])
        self.device = calls[0].device

    @classmethod
    def from_args(cls, arr, n: int, dtype: int, device, keep=None) -> "LayerGroup":
        """A group over a ready-made sow_layer_args array (the caller has validated the tensors and keeps them alive --
        `keep` -- until the launches that read the raw pointers have been enqueued)."""
        g = cls.__new__(cls)
        g.calls, g.arr, g.dtype, g.device, g._keep, g._fused, g._perms = [None] * n, arr, dtype, device, keep, None, None
        return g

    def _by_permission(self):
        """(sow_layer_args array, n, dtype) per permission value of a mixed group, in the order SOW_FUSE_ACC,
        SOW_FUSE_ACC_DEEP, none (values no layer holds are left out).  Rebuilt from
        self.arr at every call, not cached: callers and subclasses edit self.arr after construction (SharedInputGroup points
        every dx at the first), and only direct users of LayerGroup reach a mixed group -- the module surface gives siblings
        one decision."""
        out = []
        for want in (_lib.FUSE_ACC, _lib.FUSE_ACC_DEEP, 0):
            idx = [i for i, p in enumerate(self._perms) if p == want]
            if idx:
                out.append(((_lib.LayerArgs * len(idx))(*[self.arr[i] for i in idx]), len(idx), self.dtype | want))
        return out

    def forward(self) -> None:
        fn = _lib.load().sow_forward_group
        if self._fused is None:
            return _launch(self.device, "sow_forward_group", fn, self.arr, len(self.calls), self.dtype)
        for arr, n, dt in self._by_permission():
            _launch(self.device, "sow_forward_group", fn, arr, n, dt)

    def backward(self, phases: int = _lib.BWD_DATA | _lib.BWD_WEIGHTS) -> None:
        fn, phases = _lib.load().sow_backward_group, int(phases)
        if self._fused is not None and phases & _lib.BWD_DATA:
            for arr, n, dt in self._by_permission():
                _launch(self.device, "sow_backward_group", fn, arr, n, dt, _lib.BWD_DATA)
            phases &= ~_lib.BWD_DATA
            if not phases & (_lib.BWD_WEIGHTS | _lib.BWD_WEIGHTS_PARTIAL | _lib.BWD_WEIGHTS_REDUCE):
                return
        _launch(self.device, "sow_backward_group", fn, self.arr, len(self.calls), self.dtype, phases)

    def weight_gradient_plan(self, phases: int = _lib.BWD_DATA | _lib.BWD_WEIGHTS):
        """(row_owner_kernel: bool, [(slabs of x, slabs of dY) per layer]) for backward(phases) -- sow_backward_group_plan."""
        n = len(self.calls)
        slabs = (ctypes.c_int * (2 * n))()
        rc = _lib.load().sow_backward_group_plan(self.arr, n, self.dtype, int(phases), slabs)
        if rc < 0:
            _lib.check(rc, "sow_backward_group_plan")
        return bool(rc), [(slabs[2 * i], slabs[2 * i + 1]) for i in range(n)]

    def reduce_descs(self, phases: int):
        """Descriptors and block counts of the deferred weight-gradient reductions of this group (sow_reduce_batch), for a
        PARTIAL phase issued with the same `phases` flags (BWD_GROUP_SLABS included or not)."""
        lib = _lib.load()
        n, size = len(self.calls), lib.sow_reduce_desc_bytes()
        buf = ctypes.create_string_buffer(size * n)
        blocks = (ctypes.c_int * n)()
        _lib.check(lib.sow_backward_group_reduce_desc(self.arr, n, self.dtype, int(phases), buf, blocks),
                   "sow_backward_group_reduce_desc")
        return [buf.raw[i * size:(i + 1) * size] for i in range(n)], list(blocks)


class SharedInputGroup(LayerGroup):
    """Sibling calls on ONE input x2 (q / k / v, gate / up) through sow_forward_shared / sow_backward_shared: the forward
    reads x once for all of them, the data gradient is ONE dX -- the fp32 sum over the siblings rounded once, written to
    the first call's dx with its grad_beta (the other calls' dx are not written).  y, h and the weight gradients are
    bit-identical to LayerGroup.  forward() / backward() return False when the set is not admitted (the C ABI returned
    SOW_ERR_UNSUPPORTED and launched nothing); the caller then runs LayerGroup.

    Admitted: layers without accumulator (bf16 / f16, r <= 64, more than 8192 tokens), in both directions; and, in
    backward() only, siblings that ALL carry a low-rank accumulator when every call holds the SOW_FUSE_ACC permission
    (LayerCall(fuse_acc=True): the group's dtype then carries the flag) and shared_fused_acc_admits() holds: dX =
    rn(grad_beta dX + sum_i (rn(dY_i R_i^T) Q_i^T + rn(s_i dY_i B_i^T) A_i^T)), one rounding; dh and the weight gradients
    bit-identical to the flagged LayerGroup.  measured_only=True (the module surface) keeps such a set on LayerGroup --
    backward() returns False without a call -- where the shared kernel measured slower (shared_fused_acc_pays)."""

    _skip_data = False

    def __init__(self, calls: Sequence[LayerCall], measured_only: bool = False):
        super().__init__(calls)
        if len({c.args.x for c in self.calls}) != 1:
            raise ValueError("sow_amd.SharedInputGroup: every call must read the same x")
        for i in range(1, len(calls)):   # one dX for the set: the other calls' dx are not written
            self.arr[i].dx = self.arr[0].dx
        self._skip_data = (measured_only and all(c.kind == _lib.ACC_LOWRANK for c in self.calls)
                           and not shared_fused_acc_pays([c.args.r_live + c.args.r_acc for c in self.calls]))

    def _run(self, what: str, fn, *args) -> bool:
        rc = _launch_rc(self.device, fn, self.arr, len(self.calls), self.dtype, *args)
        if rc == _lib.ERR_UNSUPPORTED:
            return False
        _lib.check(rc, what)
        return True

    def forward(self) -> bool:
        return self._run("sow_forward_shared", _lib.load().sow_forward_shared)

    def backward(self, phases: int = _lib.BWD_DATA | _lib.BWD_WEIGHTS) -> bool:
        if self._skip_data and int(phases) & _lib.BWD_DATA:
            return False
        return self._run("sow_backward_shared", _lib.load().sow_backward_shared, int(phases))


class DeferredReduce:
    """The weight-gradient reductions of many layers in one launch (include/sow_amd.h: sow_reduce_batch).

    Usage per step: `sow_backward(..., phases=BWD_DATA | BWD_WEIGHTS_PARTIAL, out=..., workspace=ws_i)` for every layer
    (each layer its own workspace), then `run()` once before the gradients are consumed.  The descriptors are built on
    the first step from `add()` calls and reused while the same buffers are passed again (static training buffers, HIP
    graphs); `add()` with other pointers rebuilds them."""

    def __init__(self):
        self._keys, self._descs, self._blocks, self._dev, self._dt = [], [], [], None, None
        self._d_descs = self._d_starts = None
        self._total = 0
        self._pos = 0

    def add(self, x2, B, out, grad_beta, workspace, acc_down=None, acc_up=None, param_f32=False):
        """Register (or re-validate) the layer whose PARTIAL phase was just enqueued."""
        lib = _lib.load()
        dA, dB, dbias = out
        T, d_in = x2.shape
        r, d_out = B.shape
        kind = acc_kind(acc_down, acc_up)
        r_acc = acc_down.shape[1] if kind == _lib.ACC_LOWRANK else 0
        dt = _call_dtype(x2, param_f32, acc_down=acc_down)[0]
        key = (_ptr(dA), _ptr(dB), _ptr(dbias), T, d_in, d_out, r, r_acc, kind, float(grad_beta), dt, _ptr(workspace))
        i = self._pos
        self._pos += 1
        if i < len(self._keys) and self._keys[i] == key:
            return
        # new or changed layer: (re)build from here on
        del self._keys[i:], self._descs[i:], self._blocks[i:]
        self._d_descs = None
        buf = ctypes.create_string_buffer(lib.sow_reduce_desc_bytes())
        nb = ctypes.c_int(0)
        _lib.check(lib.sow_backward_reduce_desc(_ptr(dA), _ptr(dB), _ptr(dbias), T, d_in, d_out, r, r_acc, kind, float(grad_beta),
                                                dt, _ptr(workspace), workspace.numel(), buf, ctypes.byref(nb)),
                   "sow_backward_reduce_desc")
        self._keys.append(key)
        self._descs.append(buf.raw)
        self._blocks.append(nb.value)
        self._dev, self._dt = x2.device, dt

    def add_group(self, group: "LayerGroup", phases: int, stable_key=None):
        """Register (or re-validate) every layer of a group whose PARTIAL phase was just enqueued with `phases`.
        `stable_key`: what the reduction descriptors of the group depend on (gradient buffers, workspaces, shapes) when the
        group object and its activation pointers change from step to step -- the cached descriptors are then reused."""
        n = len(group.calls)
        key = (("group", int(phases), stable_key) if stable_key is not None
               else ("group", id(group), int(phases), bytes(group.arr)))
        i = self._pos
        self._pos += n
        if i + n <= len(self._keys) and all(self._keys[i + k] == (key, k) for k in range(n)):
            return
        del self._keys[i:], self._descs[i:], self._blocks[i:]
        self._d_descs = None
        descs, blocks = group.reduce_descs(phases)
        for k in range(n):
            self._keys.append((key, k))
            self._descs.append(descs[k])
            self._blocks.append(blocks[k])
        self._dev, self._dt = group.device, group.dtype

    def run(self):
        """One launch for every layer added since the last run()."""
        n = self._pos
        self._pos = 0
        if n == 0:
            return
        if n != len(self._keys):           # fewer layers than last step
            del self._keys[n:], self._descs[n:], self._blocks[n:]
            self._d_descs = None
        if self._d_descs is None:
            raw = b"".join(self._descs)
            self._d_descs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self._dev)
            starts, tot = [], 0
            for b in self._blocks:
                starts.append(tot)
                tot += b
            self._d_starts = torch.tensor(starts, dtype=torch.int32, device=self._dev)
            self._total = tot
        lib = _lib.load()
        _launch(self._dev, "sow_reduce_batch", lib.sow_reduce_batch, _ptr(self._d_descs), _ptr(self._d_starts), n, self._total,
                self._dt)


def gemm(A: torch.Tensor, B: torch.Tensor, *, trans_a: bool = False, trans_b: bool = False,
         out: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 0.0,
         bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = alpha * op(A) @ op(B) + beta * out (+ bias).  2-D row-major tensors with unit inner stride."""
    lib = _lib.load()
    dev = _need_gpu(A, B, out, bias)
    dt = _dt(A)
    if B.dtype != A.dtype:
        raise TypeError("sow_amd.gemm: operand dtypes differ")
    if A.dim() != 2 or B.dim() != 2:
        raise ValueError("sow_amd.gemm expects 2-D tensors")
    if A.stride(1) != 1:
        A = A.contiguous()
    if B.stride(1) != 1:
        B = B.contiguous()
    M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
    Kb, N = (B.shape[1], B.shape[0]) if trans_b else B.shape
    if K != Kb:
        raise ValueError(f"sow_amd.gemm: inner dimensions differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=dev)
        beta = 0.0
    elif tuple(out.shape) != (M, N) or out.stride(1) != 1 or out.dtype != A.dtype:
        raise ValueError("sow_amd.gemm: bad output tensor")
    if M == 0 or N == 0:
        return out
    if K == 0:
        if beta == 0.0:
            out.zero_()
        return out
    # short bf16 products split K over workgroups and need scratch for the partial sums (0 for every other shape)
    key = (M, N, K, bool(trans_a), dt)
    nws = _GEMM_WS_BYTES.get(key)
    if nws is None:
        nws = _GEMM_WS_BYTES[key] = int(lib.sow_gemm_workspace_bytes(M, N, K, int(trans_a), dt))
    ws = _ws(nws, dev) if nws else None
    _launch(dev, "sow_gemm_ex", lib.sow_gemm_ex, _ptr(A), max(A.stride(0), 1), int(trans_a), _ptr(B), max(B.stride(0), 1),
            int(trans_b), _ptr(out), max(out.stride(0), 1), _ptr(bias), M, N, K, float(alpha), float(beta), dt, _ptr(ws),
            0 if ws is None else ws.numel())
    return out


def qr_thin(W: torch.Tensor, k: int, need_r: bool = True, out_dtype: Optional[torch.dtype] = None):
    """Q[:, :k], R[:k, :] of the Householder QR of W (LAPACK sign convention), fp32 internals."""
    lib = _lib.load()
    dev = _need_gpu(W)
    if W.dim() != 2:
        raise ValueError("qr_thin expects a matrix")
    if W.stride(1) != 1:
        W = W.contiguous()
    m, n = W.shape
    out_dtype = out_dtype or W.dtype
    if k < 1 or k > m:
        raise ValueError(f"qr_thin: k={k} out of range for {m} rows")
    Q = torch.empty((m, k), dtype=out_dtype, device=dev)
    R = torch.empty((k, n), dtype=out_dtype, device=dev) if need_r else None
    nws = lib.sow_qr_workspace_bytes(m, n, k, _dt(W), int(need_r))
    ws = _ws(nws, dev)
    _launch(dev, "sow_qr_thin", lib.sow_qr_thin, _ptr(W), W.stride(0), m, n, _dt(W), k, _ptr(Q), k, _ptr(R), n, _DT[out_dtype],
            _ptr(ws), ws.numel())
    return Q, R


def cast(t: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t converted to `dtype` (float32 / bfloat16 / float16; RNE when narrowing) by sow_cast_copy: the fp32 input of a layer
    under autocast and its gradient, without an ATen cast on the hot path.  `out`: a contiguous buffer of t's shape."""
    lib = _lib.load()
    dev = _need_gpu(t, out)
    t = t.contiguous()
    if out is None:
        out = torch.empty(t.shape, dtype=dtype, device=dev)
    elif out.shape != t.shape or out.dtype != dtype or not out.is_contiguous():
        raise ValueError("sow_amd.cast: bad output tensor")
    if t.numel():
        cols = t.shape[-1] if t.dim() else 1
        rows = t.numel() // cols
        _launch(dev, "sow_cast_copy", lib.sow_cast_copy, _ptr(t), cols, _dt(t), _ptr(out), cols, _DT[dtype], rows, cols)
    return out


def zero_(tensors: Sequence[torch.Tensor]) -> None:
    """Zero a list of dense device tensors with one (or a few) multi-tensor launches."""
    lib = _lib.load()
    ts = [t for t in tensors if t is not None and t.numel() > 0]
    if not ts:
        return
    dev = _need_gpu(*ts)
    for t in ts:
        if not t.is_contiguous():
            raise ValueError("sow_amd.zero_: tensors must be contiguous")
    n = len(ts)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    sizes = (ctypes.c_int64 * n)(*[t.numel() * t.element_size() for t in ts])
    _launch(dev, "sow_zero_state", lib.sow_zero_state, ptrs, sizes, n)


def adamw_flat_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, *, lr: float,
                betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01, step: int = 1,
                grad_scale: float = 1.0) -> None:
    lib = _lib.load()
    dev = _need_gpu(param, grad, exp_avg, exp_avg_sq)
    _launch(dev, "sow_adamw_flat", lib.sow_adamw_flat, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), lr,
            betas[0], betas[1], eps, weight_decay, int(step), grad_scale, _dt(param), _dt(exp_avg))


def adamw_flat_seg_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, segments, *,
                    betas=(0.9, 0.999), eps: float = 1e-8, grad_scale: float = 1.0) -> None:
    """AdamW over segments of the flat buffers (include/sow_amd.h: sow_adamw_flat_seg).  `segments`: (begin, end, lr,
    weight_decay, step) per segment, in elements, sorted and disjoint; everything outside them is left untouched."""
    lib = _lib.load()
    dev = _need_gpu(param, grad, exp_avg, exp_avg_sq)
    n = len(segments)
    if not (param.numel() == grad.numel() == exp_avg.numel() == exp_avg_sq.numel()):
        raise ValueError("sow_amd.adamw_flat_seg_: the four buffers must have one length")
    if any(int(e) > param.numel() for _, e, *_ in segments):
        raise ValueError("sow_amd.adamw_flat_seg_: a segment ends past the buffers")
    arr = (_lib.AdamwSegment * max(n, 1))(*[_lib.AdamwSegment(int(b), int(e), float(lr), float(wd), int(st))
                                            for b, e, lr, wd, st in segments])
    _launch(dev, "sow_adamw_flat_seg", lib.sow_adamw_flat_seg, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), arr, n,
            betas[0], betas[1], eps, grad_scale, _dt(param), _dt(exp_avg))


class GradStats:
    """The 32-byte device record of ops.grad_stats_flat (include/sow_amd.h: sow_grad_stats).  Every property is a 0-dim
    view of the record in device memory: reading one launches nothing and does not synchronise; `.item()` on it does.
    sq_norm (float64): sum of g^2 of the flat buffer as stored; total_norm, clip_coef, grad_mult (float32) and nonfinite
    (int32) as the header describes them.  grad_scale: the host multiplier the record was formed with (grad_scale /
    loss_scale for a host loss_scale); counters: the skip-counter tensor its nonfinite flag was added to, or None."""

    NBYTES = ctypes.sizeof(_lib.GradStatsRecord)

    def __init__(self, buf: torch.Tensor, grad_scale: float = 1.0, counters: Optional[torch.Tensor] = None):
        if buf.dtype != torch.uint8 or buf.numel() != self.NBYTES or not buf.is_contiguous():
            raise ValueError("GradStats: the record is 32 contiguous bytes (torch.uint8)")
        self.buf, self.grad_scale, self.counters = buf, float(grad_scale), counters

    def _field(self, name: str, dtype) -> torch.Tensor:
        f = getattr(_lib.GradStatsRecord, name)       # the field's place in the C struct
        return self.buf[f.offset:f.offset + f.size].view(dtype).view(())

    sq_norm = property(lambda self: self._field("sumsq", torch.float64))
    total_sq = property(lambda self: self._field("total_sq", torch.float64))
    total_norm = property(lambda self: self._field("total_norm", torch.float32))
    clip_coef = property(lambda self: self._field("clip_coef", torch.float32))
    grad_mult = property(lambda self: self._field("grad_mult", torch.float32))
    nonfinite = property(lambda self: self._field("nonfinite", torch.int32))


_GRAD_STATS_WS: dict = {}       # device -> workspace: one per device, sized for any n


def _device_scalar(t, dtype, dev, what: str) -> Optional[torch.Tensor]:
    """A 1-element device tensor of `dtype` from a tensor (converted on the device when its dtype differs) or a number."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        return torch.full((1,), float(t), dtype=dtype, device=dev)
    if t.numel() != 1:
        raise ValueError(f"sow_amd.grad_stats_flat: {what} must have one element")
    _need_gpu(t)
    return t.reshape(1).to(dtype).contiguous()


def grad_stats_flat(grad: torch.Tensor, *, grad_scale: float = 1.0, max_norm: Optional[float] = None, extra_sq_norm=None,
                    loss_scale=None, found_inf=None, skip_counters: Optional[torch.Tensor] = None,
                    out: Optional[GradStats] = None) -> GradStats:
    """Global gradient statistics of one flat buffer, on the device (include/sow_amd.h: sow_grad_stats_flat): the squared
    norm of `grad`, total_norm = sqrt(mult0^2 * sq_norm + extra_sq_norm) with mult0 = grad_scale / loss_scale, clip_coef =
    min(1, max_norm / (total_norm + 1e-6)) (exactly 1 for max_norm None, 0 or inf), grad_mult = mult0 * clip_coef and the
    nonfinite flag (total_norm not finite, or found_inf != 0).  Two launches on the current stream, no host read.
    extra_sq_norm: the squared norm of gradients that live elsewhere (a device tensor; float64 is taken as it is);
    loss_scale: a float (folded into grad_scale on the host) or a 1-element float32 device tensor; found_inf: a 1-element
    float32 device tensor (torch.amp's convention: non-zero = overflow seen); skip_counters: an int32 device tensor, every
    entry raised by the flag; out: a GradStats to write into (a fresh record otherwise).
    The partial sums go through ONE cached workspace per device: calls on one stream are ordered by it, calls on two
    streams of one device that may overlap race on that workspace -- order such streams with an event."""
    lib = _lib.load()
    dev = _need_gpu(grad, skip_counters, None if out is None else out.buf)
    if not grad.is_contiguous():
        raise ValueError("sow_amd.grad_stats_flat: the gradient buffer must be contiguous")
    mult = float(grad_scale)
    ls = None
    if isinstance(loss_scale, torch.Tensor):
        ls = _device_scalar(loss_scale, torch.float32, dev, "loss_scale")
    elif loss_scale is not None:
        mult = mult / float(loss_scale)
    extra = _device_scalar(extra_sq_norm, torch.float64, dev, "extra_sq_norm")
    finf = _device_scalar(found_inf, torch.float32, dev, "found_inf")
    if skip_counters is not None and (skip_counters.dtype != torch.int32 or not skip_counters.is_contiguous()):
        raise TypeError("sow_amd.grad_stats_flat: skip_counters must be a contiguous int32 tensor")
    ws = _GRAD_STATS_WS.get(dev)
    if ws is None:      # the query is monotone in n and capped: what it asks for the largest n serves every n
        ws = _GRAD_STATS_WS[dev] = torch.empty(lib.sow_grad_stats_workspace_bytes(2 ** 62), dtype=torch.uint8, device=dev)
    if out is None:
        out = GradStats(torch.empty(GradStats.NBYTES, dtype=torch.uint8, device=dev))
    out.grad_scale, out.counters = mult, skip_counters
    _launch(dev, "sow_grad_stats_flat", lib.sow_grad_stats_flat, _ptr(grad) if grad.numel() else None, grad.numel(), _dt(grad),
            mult, 0.0 if max_norm is None else float(max_norm), _ptr(extra), _ptr(ls), _ptr(finf), _ptr(skip_counters),
            0 if skip_counters is None else skip_counters.numel(), _ptr(ws), ws.numel(), _ptr(out.buf))
    return out


def adamw_flat_seg_stats_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, segments,
                          stats: GradStats, *, betas=(0.9, 0.999), eps: float = 1e-8, seg_counter=None,
                          skip_counters: Optional[torch.Tensor] = None, skip_nonfinite: bool = False) -> None:
    """adamw_flat_seg_ with the gradient multiplier read from `stats` on the device (include/sow_amd.h:
    sow_adamw_flat_seg_stats).  skip_nonfinite: a record whose nonfinite flag is set leaves param and both moments as they
    are.  seg_counter: per segment an index into the int32 device tensor skip_counters (-1: none); a segment whose counter
    reads c > 0 steps with the bias correction of step max(1, step - c)."""
    lib = _lib.load()
    dev = _need_gpu(param, grad, exp_avg, exp_avg_sq, stats.buf, skip_counters)
    n = len(segments)
    if not (param.numel() == grad.numel() == exp_avg.numel() == exp_avg_sq.numel()):
        raise ValueError("sow_amd.adamw_flat_seg_stats_: the four buffers must have one length")
    if any(int(e) > param.numel() for _, e, *_ in segments):
        raise ValueError("sow_amd.adamw_flat_seg_stats_: a segment ends past the buffers")
    if seg_counter is not None and len(seg_counter) != n:
        raise ValueError("sow_amd.adamw_flat_seg_stats_: seg_counter needs one entry per segment")
    if skip_counters is not None and (skip_counters.dtype != torch.int32 or not skip_counters.is_contiguous()):
        raise TypeError("sow_amd.adamw_flat_seg_stats_: skip_counters must be a contiguous int32 tensor")
    arr = (_lib.AdamwSegment * max(n, 1))(*[_lib.AdamwSegment(int(b), int(e), float(lr), float(wd), int(st))
                                            for b, e, lr, wd, st in segments])
    cnt = None if seg_counter is None else (ctypes.c_int * max(n, 1))(*[int(c) for c in seg_counter])
    _launch(dev, "sow_adamw_flat_seg_stats", lib.sow_adamw_flat_seg_stats, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
            arr, cnt, n, betas[0], betas[1], eps, _ptr(stats.buf), int(bool(skip_nonfinite)), _ptr(skip_counters),
            0 if skip_counters is None else skip_counters.numel(), _dt(param), _dt(exp_avg))


def ttadam_dense_(param, grad, exp_avg, exp_avg_sq, *, beta1, beta2, eps, step_size, lr_times_wd, clamp_v: bool) -> None:
    lib = _lib.load()
    dev = _need_gpu(param, grad, exp_avg, exp_avg_sq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError("ttadam_dense_ expects contiguous float32 tensors")
    _launch(dev, "sow_ttadam_dense", lib.sow_ttadam_dense, _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
            beta1, beta2, eps, step_size, lr_times_wd, int(clamp_v))


def tt_kron_core(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """einsum('aijb,cijd->acijbd') reshaped to [ra*rc, i, j, rb*rd] (reference tt.py:469-475)."""
    lib = _lib.load()
    dev = _need_gpu(a, b)
    a, b = a.contiguous().float(), b.contiguous().float()
    ra0, i, j, ra1 = a.shape
    rb0, i2, j2, rb1 = b.shape
    if (i, j) != (i2, j2):
        raise ValueError("tt_kron_core: physical dimensions differ")
    out = torch.empty((ra0 * rb0, i, j, ra1 * rb1), dtype=torch.float32, device=dev)
    _launch(dev, "sow_tt_kron_core", lib.sow_tt_kron_core, _ptr(a), _ptr(b), _ptr(out), ra0, rb0, i * j, ra1, rb1)
    return out


def absmax(x: torch.Tensor) -> float:
    """max |x| of an fp32 device tensor (one small kernel + a host read)."""
    lib = _lib.load()
    dev = _need_gpu(x)
    x = x.contiguous().float()
    out = torch.empty(1, dtype=torch.float32, device=dev)
    _launch(dev, "sow_absmax", lib.sow_absmax, _ptr(x), x.numel(), _ptr(out))
    return float(out.item())


def small_inverse(mats: torch.Tensor) -> torch.Tensor:
    """Inverse of a batch of [r, r] fp32 matrices (r <= 16)."""
    lib = _lib.load()
    dev = _need_gpu(mats)
    m = mats.contiguous().float()
    b, r, r2 = m.shape
    if r != r2:
        raise ValueError("small_inverse expects square matrices")
    out = torch.empty_like(m)
    _launch(dev, "sow_small_inverse", lib.sow_small_inverse, _ptr(m), _ptr(out), b, r)
    return out


def axpby_(x: torch.Tensor, y: torch.Tensor, a: float, b: float) -> torch.Tensor:
    """y <- a*x + b*y"""
    lib = _lib.load()
    dev = _need_gpu(x, y)
    if x.dtype != y.dtype or x.numel() != y.numel() or not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("axpby_: x and y must be contiguous, same dtype and size")
    _launch(dev, "sow_axpby", lib.sow_axpby, _ptr(x), _ptr(y), x.numel(), float(a), float(b), _dt(x))
    return y


class _MatMul(torch.autograd.Function):
    """2-D a @ b on the MFMA GEMM kernel with autograd (used by the TT layer's core contractions)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return gemm(a, b)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = dc.contiguous()
        da = gemm(dc, b, trans_b=True) if ctx.needs_input_grad[0] else None   # dC @ B^T
        db = gemm(a, dc, trans_a=True) if ctx.needs_input_grad[1] else None   # A^T @ dC
        return da, db


def matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _MatMul.apply(a, b)
