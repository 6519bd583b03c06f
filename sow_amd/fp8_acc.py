"""acc_quant.py's former name: only the four names that the test files of the commit before the rename import."""
from .acc_quant import FORMATS, quantize_accumulators, quantize_tensor  # noqa: F401


def quantize_tensor_fp4(W): return quantize_tensor(W, "mxfp4")
