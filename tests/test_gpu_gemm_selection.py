"""-m gpu: which kernel writes C for a sow_gemm_ex call (trans_a = 0), at the smallest shapes where each arm of the dense
selection rule (api.hip: pick_gemm) bites, under the defaults and under the GEMM4 / GEMM3S / GEMM3 / NO_GEMM3S /
FORCE_GEMM_V1 switches.  Each case asserts the kernel's name (torch.profiler, as test_gpu_elementwise.py) and C element by
element against the float64 product with the bound of that file's GEMM cases (check_rounded: one rounding of an fp32 sum).

t256 = ceil(M / 256) ceil(N / 256), t128 likewise; operands aligned, ld = row length, no workspace (so no split over K).
The table was recorded from the library as it stood before the operand structs and the selector were introduced; the same
table holds after.  The bf16 / f16 asymmetry at 7680 x 1024 x 256 is deliberate: bf16 passes a gate (K >= 512 below 160
big tiles) before gemm4 is considered, f16 has none."""
import functools

import pytest
import torch

import test_gpu_elementwise as E
from numerics import check_rounded, fp32_floor
from sow_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
FAMILY = ("gemm_kernel", "gemm2_kernel", "gemm3_kernel", "gemm3s_kernel", "gemm4_kernel", "gemm4_f16_kernel")
SWITCHES = ("GEMM4", "GEMM3S", "GEMM3", "NO_GEMM3S", "FORCE_GEMM_V1")
BASE = (1536, 1024, 512)   # t256 = 24, t128 = 96

# (id, dtype, (M, N, K), trans_b, switches, kernel)
CASES = [
    ("base_default_bf16", BF16, BASE, False, {}, "gemm3s_kernel"),
    ("base_default_bf16_nt", BF16, BASE, True, {}, "gemm3s_kernel"),
    ("base_gemm4_bf16", BF16, BASE, False, dict(GEMM4=1), "gemm4_kernel"),
    ("base_gemm4_bf16_nt", BF16, BASE, True, dict(GEMM4=1), "gemm4_kernel"),
    ("base_gemm4_force_v1_bf16", BF16, BASE, False, dict(GEMM4=1, FORCE_GEMM_V1=1), "gemm_kernel"),
    ("base_gemm3s0_bf16", BF16, BASE, False, dict(GEMM3S=0), "gemm2_kernel"),
    ("base_gemm3s0_bf16_nt", BF16, BASE, True, dict(GEMM3S=0), "gemm2_kernel"),
    ("base_gemm3s0_gemm3_bf16", BF16, BASE, False, dict(GEMM3S=0, GEMM3=1), "gemm3_kernel"),
    ("base_no_gemm3s_bf16", BF16, BASE, False, dict(NO_GEMM3S=1), "gemm_kernel"),
    ("base_force_v1_bf16", BF16, BASE, False, dict(FORCE_GEMM_V1=1), "gemm_kernel"),
    ("base_default_f16", F16, BASE, False, {}, "gemm_kernel"),
    ("base_gemm4_f16", F16, BASE, False, dict(GEMM4=1), "gemm4_f16_kernel"),
    ("base_gemm4_force_v1_f16", F16, BASE, False, dict(GEMM4=1, FORCE_GEMM_V1=1), "gemm_kernel"),
    ("k504_bf16", BF16, (1536, 1024, 504), False, {}, "gemm_kernel"),              # K < 512 below 160 big tiles
    ("t128_88_bf16", BF16, (1408, 1024, 512), False, {}, "gemm_kernel"),           # t128 = 88 < 96
    ("t256_120_bf16", BF16, (7680, 1024, 512), False, {}, "gemm4_kernel"),         # t256 = 120
    ("t256_120_f16", F16, (7680, 1024, 512), False, {}, "gemm4_f16_kernel"),
    ("t256_120_k256_bf16", BF16, (7680, 1024, 256), False, {}, "gemm_kernel"),     # the bf16 gate comes before gemm4 ...
    ("t256_120_k256_f16", F16, (7680, 1024, 256), False, {}, "gemm4_f16_kernel"),  # ... and f16 has no gate
    ("t256_160_k56_bf16", BF16, (10240, 1024, 56), False, {}, "gemm2_kernel"),     # t256 = 160, K < 64: gemm4 does not take it
    ("t256_160_k2048_nogemm4_bf16", BF16, (10240, 1024, 2048), False, dict(GEMM4=0), "gemm3_kernel"),
    ("t256_160_k1024_nogemm4_bf16", BF16, (10240, 1024, 1024), False, dict(GEMM4=0), "gemm2_kernel"),
]


@functools.lru_cache(maxsize=2)   # cases of one shape and dtype are neighbours in CASES
def _operands(dtype, M, N, K):
    """a [M, K], b [K, N], bias [N] on the GPU in `dtype`, and on the CPU the float64 reference a b + bias with the fp32
    accumulation floor of check_rounded.  Shared by the cases of a shape; nobody writes to them."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(dtype).to(DEV)
    b = (torch.randn(K, N, generator=g) * 0.05).to(dtype).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(dtype).to(DEV)
    a64, b64 = a.double(), b.double()
    ref = (a64 @ b64 + bias.double()).cpu()
    acc = fp32_floor(((a64 * a64) @ (b64 * b64)).cpu(), K)
    return a, b, bias, ref, acc


@pytest.mark.parametrize("name,dtype,shape,nt,switches,kernel", CASES, ids=[c[0] for c in CASES])
def test_gemm_selection(name, dtype, shape, nt, switches, kernel):
    lib = _lib.load()
    M, N, K = shape
    a, b, bias, ref, acc = _operands(dtype, M, N, K)
    bmat = b.t().contiguous() if nt else b
    C = torch.full((M, N), float("nan"), dtype=dtype, device=DEV)
    dt = _lib.BF16 if dtype == BF16 else _lib.F16

    def call():
        _lib.check(lib.sow_gemm_ex(a.data_ptr(), K, 0, bmat.data_ptr(), K if nt else N, int(nt), C.data_ptr(), N,
                                   bias.data_ptr(), M, N, K, 1.0, 0.0, dt, None, 0, E._stream()), "sow_gemm_ex")

    with _lib.switch(**switches):
        seq = E._kernel_seq(call)
    assert all(lib.sow_get_switch(k.encode()) == -1 for k in SWITCHES)
    ran = [k for k in FAMILY if E._has_kernel(seq, k)]
    print(f"{name}: {ran}")
    assert ran == [kernel], f"{name}: expected {kernel} alone, the trace shows {ran}: {sorted(set(seq))}"
    st = check_rounded(C.cpu(), ref, dtype, acc=acc, name=name)
    print(f"{name}: worst err/limit {st['worst']:.3f}, inexact {100 * st['inexact']:.4f} %")
