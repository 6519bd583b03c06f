"""One wide-rank layer (T = 32768, d_in = d_out = 2048, r = 200, bf16), forward + backward through the C ABI wrappers, for
`rocprofv3 --kernel-trace --stats`.  Argument: 1 = NO_WIDE_CHAIN on (the generic GEMM composition), 0 = the fused kernels.

    rocprofv3 --kernel-trace --stats -d out -o run -- python tools/wide_rank_trace.py 0
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sow_amd import _lib, ops  # noqa: E402


def main():
    generic = len(sys.argv) > 1 and sys.argv[1] == "1"
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lib = _lib.load()
    assert lib.sow_set_switch(b"NO_WIDE_CHAIN", 1 if generic else 0) == 0
    T, d, r, dt = 32768, 2048, 200, torch.bfloat16
    torch.manual_seed(0)
    x = torch.randn(T, d, device="cuda", dtype=dt)
    A = (torch.randn(d, r, device="cuda") * 0.02).to(dt)
    B = (torch.randn(r, d, device="cuda") * 0.07).to(dt)
    bias = torch.randn(d, device="cuda", dtype=dt)
    dy = torch.randn(T, d, device="cuda", dtype=dt)
    ws = torch.empty(ops.workspace_bytes(T, d, d, r, 0, _lib.ACC_NONE, dt), dtype=torch.uint8, device="cuda")
    out = (torch.empty(d, r, device="cuda", dtype=dt), torch.empty(r, d, device="cuda", dtype=dt),
           torch.empty(d, device="cuda", dtype=dt))
    dx = torch.empty_like(x)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for i in range(iters + 3):
        if i == 3:
            ev[0].record()
        y, h = ops.sow_forward(x, A, B, None, None, bias, 0.75)
        ops.sow_backward(dy, x, h, A, B, None, None, 0.75, True, out=out, dx=dx, workspace=ws)
    ev[1].record()
    torch.cuda.synchronize()
    print(f"{'generic' if generic else 'wide'}: forward + backward {ev[0].elapsed_time(ev[1]) * 1000 / iters:.1f} us per step")


if __name__ == "__main__":
    main()
