"""The reference of the 16-bit (bf16 / fp16) SpMM tests: the oracle on the widened operand, rounded once by torch's CPU cast.

`x16.float()` is exact, the oracle forms products, sums and the mean's division in fp32, and CPU `.to(dtype)` rounds to nearest even,
keeps NaN / Inf (and bf16 subnormals) and sends an fp16 overflow to Inf -- tests/test_half_host.py pins those properties."""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
UNIT_ROUNDOFF = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def round16(a, dtype) -> torch.Tensor:
    """An fp32 array rounded once to `dtype` (a CPU tensor)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)


def to16(a, dtype) -> torch.Tensor:
    """Test operands: an fp32 array as a `dtype` CPU tensor (the values the kernel is given)."""
    return round16(a, dtype)


def widen(t16: torch.Tensor) -> np.ndarray:
    return t16.to(torch.float32).numpy()


def reference(oracle, rowptr, col, val, x16: torch.Tensor, reduce):
    """(ref32, ref16): the oracle's fp32 result on the widened operand, and that rounded once to x16's dtype."""
    ref32, _ = oracle.spmm_fw(rowptr, col, val, widen(x16), reduce)
    return ref32, round16(ref32, x16.dtype)


def bits(t: torch.Tensor) -> np.ndarray:
    """The 16-bit patterns of a bf16 / fp16 tensor."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def rounding_bound(ref32, tol, dtype):
    """Per-element bound on |got - ref32| for a result rounded once to `dtype`: another summation order moves the fp32 value by at most
    `tol` (cases.sum_tolerance), and rounding to nearest adds at most one unit roundoff of the value rounded; fp16 also has an absolute
    half-spacing of its subnormals, 2^-25."""
    u = UNIT_ROUNDOFF[dtype]
    return tol + u * (np.abs(ref32) + tol) + (2.0 ** -25 if dtype == torch.float16 else 0.0)
