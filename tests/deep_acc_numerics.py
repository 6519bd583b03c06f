"""Cases of the fused low-rank-accumulator pass past 256 columns (SOW_FUSE_ACC_DEEP, chain_deep_acc.hip) -- a plain module
shared by tests/test_gpu_deep_acc.py and tests/test_deep_acc_numerics_cpu.py.

The contract is the one tests/fused_acc_numerics.py states (h_acc = rn(x Q), h_save = rn(s x A), y = rn(h_acc R + h_save B +
bias), the mirror for dX: ONE output rounding), so the cases are built with its `case` and held to its `check`; `emulate` and
`r_pad` there are general in r_acc + r.  What is new is the tile code: r_pad = ceil64(r_acc + r) columns of H in groups of
256, panels side by side in LDS, 256 < r_acc + r <= 960.
"""
import fused_acc_numerics as FA

BF16, F16 = FA.BF16, FA.F16
case, check, emulate, r_pad = FA.case, FA.check, FA.emulate, FA.r_pad

# (T, d_in, d_out, r_live, r_acc): the smallest shapes that reach every edge of the column-group code
CASES = [
    # the second group holds 2 real columns of its 64; ragged last token block
    case("tot258", BF16, 193, 72, 264, 58, 200),
    # the live columns 230 .. 279 cross the group boundary at 256
    case("straddle_256", BF16, 130, 264, 72, 50, 230, bias=False),
    # live = one whole panel (the second group), no ones column; the 80 KiB plan, two workgroups per CU
    case("tot320_r64", BF16, 129, 136, 264, 64, 256),
    # two full groups
    case("tot512", BF16, 65, 264, 136, 64, 448),
    case("tot300_f16", F16, 257, 264, 72, 50, 250),
    # 15 panels, exactly 160 KiB: four groups, the last of 192 columns
    case("tot960", BF16, 65, 136, 72, 50, 910),
    case("tot960_f16", F16, 65, 72, 136, 50, 910, bias=False),
    # a single token
    case("one_token_tot400", BF16, 1, 264, 520, 16, 384, bias=False),
    # one K step, widths below one tile
    case("k8_tot258", BF16, 64, 8, 24, 2, 256),
    # a llama_60m layer (512 -> 1376) at its ninth accumulate
    case("llama60m_racc450", BF16, 257, 512, 1376, 50, 450, s=0.5),
]
BY_NAME = {c.name: c for c in CASES}
