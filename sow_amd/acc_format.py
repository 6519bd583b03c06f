"""Where a quantised-accumulator format is described: one record per format, read by ops.py (checks, shapes, C entry points,
dispatch rule) and acc_quant.py (the quantiser).  What adding a format takes is listed in DESIGN.md section 4.5c."""
from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import _lib

SKINNY_MAX_T = 32          # include/sow_amd.h: sow_forward_skinny admits at most 32 tokens per layer


def skinny_fp8_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule for an E4M3 accumulator (profiles/fp8_acc.txt), the one place that
    encodes it: the calls at which streaming the codes (q) is faster than the image pass followed by the bf16 skinny forward
    on the image (d).  Measured (us, r = 50, T = 4 / 32): 4096->4096 25.4 / 32.9 against 40.8 / 44.2, 4096->11008 37.6 / 47.4
    against 67.4 / 92.6, 11008->4096 37.4 / 47.4 against 67.8 / 83.7, 512->512 17.7 / 19.8 against 20.5 / 22.2, q + k + v of
    4096->4096 39.9 / 59.3 against 73.7 / 88.0; q / d lies between 0.47 and 0.89 in all 48 rows (T = 1, 4, 16, 32; r = 8, 50):
    the rule excludes nothing.  NOT measured: f16, widths above 11008."""
    return 1 <= T <= SKINNY_MAX_T


def skinny_fp4_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule for an MXFP4 accumulator (profiles/fp4_acc.txt), the one place that
    encodes it: the calls at which streaming the codes (q4) is faster than the image pass followed by the bf16 skinny forward on
    the image (d4) by more than the run-to-run spread of the row.  Measured (us, r = 50, T = 4 / 32; +- the larger spread
    of the two variants): 4096->4096 21.1 / 29.9 against 39.7 / 43.0 (+- 2.5 / 2.6), 4096->11008 24.3 / 38.4 against 62.9 / 90.1
    (+- 1.8 / 2.8), 11008->4096 26.5 / 37.4 against 62.3 / 81.0 (+- 1.6 / 1.9), 512->512 14.5 / 16.3 against 18.3 / 19.2 (+- 1.5 / 0.3),
    q + k + v of 4096->4096 33.5 / 52.4 against 70.3 / 84.5 (+- 0.7 / 1.0); q4 / d4 lies between 0.37 and 0.85 in all 48 rows (T = 1,
    4, 16, 32; r = 8, 50) and the gap exceeds the spread in each: the rule excludes nothing.  q4 is never slower than the E4M3
    codes (q4 / q8 0.68 ... 1.00); it loses to the bf16 accumulator at 4096->4096, T = 32, r = 8 (29.1 against 25.4) and by up to
    10 % on 512-wide layers at r = 8, which does not enter the rule: the kind buys memory there.  NOT measured: f16, widths above
    11008."""
    return 1 <= T <= SKINNY_MAX_T


SKINNY_ROWS_MAX = 64       # include/sow_amd.h: sow_forward_skinny_rows admits at most 64 (sow_amd.skinny_rows opts in)


def skinny_fp8_rows_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule for an E4M3 accumulator at 33 ... 64 rows inside sow_amd.skinny_rows (profiles/skinny_rows.txt,
    DESIGN.md section 4.5d), the one place that encodes it: the calls at which sow_forward_skinny_rows on the codes (n) is
    faster than the image pass followed by sow_forward / sow_forward_group on the image (a) by more than the larger
    run-to-run spread of the two.  Measured (us, r = 50, T = 33 / 64; +- the larger spread): 4096->4096 42.8 /
    51.6 against 237.9 / 134.5 (+- 2.3 / 3.0), 4096->11008 67.4 / 80.8 against 394.4 / 147.0 (+- 1.8 / 1.3), 11008->4096 65.2 / 82.9
    against 462.2 / 314.6 (+- 0.8 / 0.5), 512->512 21.0 / 23.2 against 44.1 / 42.2 (+- 1.2 / 11.1), q + k + v of 4096->4096 76.5 / 96.5
    against 692.3 / 381.1 (+- 2.8 / 0.3); a / n lies between 1.63 and 9.05 in all 36 rows and the gap exceeds the spread in each: the
    rule excludes nothing.  Against two sow_forward_skinny calls on the row halves (b2) n wins or ties except 11008->4096, T = 64,
    r = 8 (73.5 against 71.5 +- 1.3), which does not enter the rule.  NOT measured: f16, widths above 11008."""
    return SKINNY_MAX_T < T <= SKINNY_ROWS_MAX


def skinny_fp4_rows_pays(T: int, d_in: int, d_out: int) -> bool:
    """The same rule for an MXFP4 accumulator (profiles/skinny_rows.txt).  Measured
    (us, r = 50, T = 33 / 64; +- the larger spread): 4096->4096 39.6 / 49.1 against 236.1 / 131.0 (+- 1.4 / 1.8), 4096->11008 59.2 /
    77.2 against 391.9 / 144.7 (+- 2.6 / 1.8), 11008->4096 58.8 / 78.0 against 458.9 / 306.7 (+- 1.3 / 1.2), 512->512 20.2 / 22.7 against
    45.4 / 44.2 (+- 0.9 / 6.9), q + k + v of 4096->4096 71.3 / 92.0 against 691.4 / 378.8 (+- 2.6 / 1.5); a / n lies between 1.66 and 9.70
    in all 36 rows and the gap exceeds the spread in each: the rule excludes nothing.  Two sow_forward_skinny calls on the row halves
    (b2) are faster than n at T = 64 on 11008->4096 (60.7 against 69.2 at r = 8, 74.7 against 78.0 at r = 50) and on 4096->11008 at
    r = 8 (70.7 against 73.6): reported in DESIGN with the kernel trace of one
    of them (phase A 63.3 us against 2 x 28.5), no split routing is built.  NOT measured: f16, widths above 11008."""
    return SKINNY_MAX_T < T <= SKINNY_ROWS_MAX


# (d_in, d_out) -> the most rows at which the pair on the codes won: the tables of the two docstrings below
SHORT_CODES_TABLE: dict = {"fp8_e4m3": {(3072, 768): 128, (4096, 4096): 128, (4096, 11008): 128, (11008, 4096): 128},
                           "mxfp4": {(3072, 768): 128, (4096, 4096): 128, (4096, 11008): 128, (11008, 4096): 128, (512, 512): 512,
                                     (512, 1376): 512}}


def _short_codes_pays(name: str, T: int, d_in: int, d_out: int) -> bool:
    return 64 < T <= SHORT_CODES_TABLE[name].get((d_in, d_out), 0)


def short_fp8_pays(T: int, d_in: int, d_out: int) -> bool:
    """The measured dispatch rule for an E4M3 accumulator in calls WITH gradients inside sow_amd.short_rows + sow_amd.short_codes
    (profiles/short_codes.txt), the one place that encodes it: the (rows, shape) classes at which forward +
    data gradient on the codes read in place (n: sow_forward_short_codes / sow_backward_short_codes) beat what such a layer runs
    without the opt-in (a: the image pass ahead of the forward and again ahead of the data gradient, and on the image the short pair
    where short_rows_pays admits the row, else sow_forward / the data phase of sow_backward_ex) by more than the larger run-to-run
    spread of the two, at r = 8 AND r = 50.  One line per measured shape, the most rows up to which n won at every measured row count
    (65, 128, 256, 512, 1024) from 65 on; 0 = never (bf16, MI355X):

        768->768: T <= 0
        768->3072: T <= 0
        3072->768: T <= 128
        4096->4096: T <= 128
        4096->11008: T <= 128
        11008->4096: T <= 128
        512->512: T <= 0
        512->1376: T <= 0

    Measured (us, a against n, +- the larger spread; r = 50 at T = 65 / 128 / 256): 3072->768 66.2 / 76.2 / 113.1 against 58.1 / 70.4 /
    116.2 (+- 3.1 / 1.8 / 1.1), 4096->4096 128.8 / 168.0 / 227.3 against 112.8 / 154.2 / 270.4 (+- 0.8 / 1.7 / 1.4), 4096->11008 237.5 /
    306.7 / 302.1 against 206.0 / 273.9 / 512.8 (+- 0.8 / 2.8 / 2.5), 11008->4096 262.7 / 352.2 / 379.1 against 235.4 / 324.4 / 610.6
    (+- 0.7 / 1.8 / 1.5): a / n is 1.08 ... 1.17 where n wins -- the two image passes, 5 ... 19 us each -- and falls to 0.11 at 1024 rows,
    where n reads the codes once per 64-row block and a has left the short pair.  On the 768- and 512-wide shapes n's median is below
    a's at every row count up to 256 (a / n 1.00 ... 1.20) but the gap is inside the spread of a row at one rank or the other (up to
    20.8 us at 768->768, T = 65), so the rule excludes them; 3072->768 loses at 256 rows and r = 50 (116.2 against 113.1).
    The rule EXCLUDES: every row count above a shape's line, every shape that was not measured, calls of at most 64 rows.  NOT
    measured: f16, a full finetune step."""
    return _short_codes_pays("fp8_e4m3", T, d_in, d_out)


def short_fp4_pays(T: int, d_in: int, d_out: int) -> bool:
    """The same rule for an MXFP4 accumulator (profiles/short_codes.txt; a, n and the criterion as in
    short_fp8_pays).  One line per measured shape:

        768->768: T <= 0
        768->3072: T <= 0
        3072->768: T <= 128
        4096->4096: T <= 128
        4096->11008: T <= 128
        11008->4096: T <= 128
        512->512: T <= 512
        512->1376: T <= 512

    Measured (us, a against n, +- the larger spread; r = 50 at T = 65 / 128 / 256): 3072->768 65.0 / 75.3 / 111.9 against 56.0 / 68.2 /
    113.2 (+- 0.5 / 1.3 / 1.2), 4096->4096 125.4 / 165.3 / 226.5 against 106.4 / 146.7 / 258.1 (+- 0.9 / 0.4 / 1.0), 4096->11008 232.2 /
    297.2 / 297.5 against 189.4 / 253.4 / 474.0 (+- 1.1 / 1.9 / 11.3), 11008->4096 260.0 / 344.3 / 378.6 against 220.7 / 307.9 / 578.8
    (+- 3.8 / 3.3 / 2.4); 512->512 at T = 65 / 128 / 256 / 512 / 1024: 42.6 / 42.8 / 50.2 / 73.3 / 74.1 against 40.0 / 40.2 / 47.6 / 61.5 /
    104.9 (+- 0.5 / 0.7 / 0.5 / 0.7 / 1.0); 512->1376: 44.7 / 47.1 / 59.6 / 84.9 / 84.8 against 41.1 / 42.8 / 55.2 / 78.6 / 141.6.  a / n is
    1.06 ... 1.23 where n wins and 0.11 at 1024 rows of 11008->4096.  On the 768-wide shapes a row's spread (up to 24.6 us at T = 65)
    hides the gap at one rank or the other: excluded.  The rule EXCLUDES what short_fp8_pays excludes.  NOT measured: f16, a full
    finetune step."""
    return _short_codes_pays("mxfp4", T, d_in, d_out)


class AccFormat(NamedTuple):
    name: str                       # the fmt= argument of quantize_accumulators
    label: str                      # the name used in messages
    kind: int                       # include/sow_amd.h: SOW_ACC_DENSE_*
    code_dtype: torch.dtype
    scale_dtype: torch.dtype
    rows_per_code: int              # rows of one column packed into a code element
    block: Optional[int]            # rows of one column per scale; None: one scale per column
    d_in_multiple: int              # the widths quantize_accumulators converts and the streaming kernels admit
    d_out_multiple: int
    workspace_query: str            # C entry (T, d_in, d_out, r, dtype) -> bytes of the skinny forward on the codes
    dequantize: str                 # C entry that writes the image
    exp_range: dict                 # compute dtype -> the (lo, hi) clamp of a scale's exponent
    scale_bias: int                 # a scale is stored as its exponent + this
    code_max: float                 # the largest code magnitude
    frexp: Tuple[float, int]        # code_max = threshold * 2^offset with threshold in [0.5, 1)
    pays: Callable[[int, int, int], bool]      # the measured rule that admits the streaming path
    pays_rows: Callable[[int, int, int], bool]     # ... at 33 ... 64 rows (sow_forward_skinny_rows inside sow_amd.skinny_rows)
    # ... of calls WITH gradients at 65 ... 1024 rows on the codes read in place (sow_forward_short_codes / sow_backward_short_codes
    # inside sow_amd.short_rows + sow_amd.short_codes).  Last and with a default: a record built without it routes nothing there
    pays_short: Callable[[int, int, int], bool] = lambda T, d_in, d_out: False

    def code_shape(self, d_in, d_out): return (d_in // self.rows_per_code, d_out)      # (of a [d_in, d_out] matrix, as scale_shape)
    def scale_shape(self, d_in, d_out): return (d_out,) if self.block is None else (d_in // self.block, d_out)
    def logical_shape(self, codes): return (codes.shape[0] * self.rows_per_code, codes.shape[1])

    def scales_fit(self, scales, d_in, d_out):
        """`scales` are this format's scales of a [d_in, d_out] matrix (written out, one .shape read: it runs on every generated token)."""
        b = self.block
        return (scales.dtype == self.scale_dtype and (b is None or d_in % b == 0)
                and tuple(scales.shape) == ((d_out,) if b is None else (d_in // b, d_out)))

    def well_formed(self, codes, scales):
        """(codes, scales) are a pair of this format: 2-D codes, and the scales of the matrix they stand for."""
        cs = codes.shape
        return len(cs) == 2 and self.scales_fit(scales, cs[0] * self.rows_per_code, cs[1])


FORMATS = {f.name: f for f in (
    # W^[k, n] = codes[k, n] * 2^scales[n]
    AccFormat(name="fp8_e4m3", label="E4M3", kind=_lib.ACC_DENSE_FP8, code_dtype=torch.float8_e4m3fn, scale_dtype=torch.int8,
              rows_per_code=1, block=None, d_in_multiple=8, d_out_multiple=8, workspace_query="sow_forward_skinny_fp8_workspace_bytes",
              dequantize="sow_acc_dequantize", exp_range={torch.bfloat16: (-117, 119), torch.float16: (-15, 7)}, scale_bias=0,
              code_max=448.0, frexp=(0.875, 9), pays=skinny_fp8_pays, pays_rows=skinny_fp8_rows_pays, pays_short=short_fp8_pays),
    # W^[k, n] = e2m1(nibble k % 2 of codes[k / 2, n]) * 2^(scales[k / 32, n] - 127): E8M0 scale bytes
    AccFormat(name="mxfp4", label="MXFP4", kind=_lib.ACC_DENSE_FP4, code_dtype=torch.uint8, scale_dtype=torch.uint8,
              rows_per_code=2, block=32, d_in_multiple=32, d_out_multiple=8, workspace_query="sow_forward_skinny_fp4_workspace_bytes",
              dequantize="sow_acc_dequantize_fp4", exp_range={torch.bfloat16: (-125, 125), torch.float16: (-13, 13)}, scale_bias=127,
              code_max=6.0, frexp=(0.75, 3), pays=skinny_fp4_pays, pays_rows=skinny_fp4_rows_pays, pays_short=short_fp4_pays),
)}
BY_CODE_DTYPE = {f.code_dtype: f for f in FORMATS.values()}
BY_KIND = {f.kind: f for f in FORMATS.values()}
