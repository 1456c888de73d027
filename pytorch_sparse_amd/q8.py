"""SpMM over quantised features: ``x`` held as OCP fp8 (``torch.float8_e4m3fn``) codes with one float32 scale per row
(csrc/spmm_q8.hip, csrc/ops_q8.cpp).

The gather of ``x[col[e], :]`` is what ``matmul`` pays for.  Layer-0 features of a large graph are constants of a run
and need no gradient: at one byte per element a 128-wide row is one cache line, where bfloat16 moves two and float32
four.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

from .tensor import SparseTensor

_MAX_F = 1024


def quantize_rows(x: Tensor) -> Tuple[Tensor, Tensor]:
    """``x [N, F]`` (float32, bfloat16 or float16, on the GPU) -> ``(xq [N, F] float8_e4m3fn, scale [N] float32)`` with
    ``scale[n] = absmax(x[n, :]) / 448`` (``1`` for a row of zeros) and
    ``xq = (x.float() / scale[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn)``: an IEEE float32 divide and
    round-to-nearest-even, code for code what torch computes for that expression on the CPU.  Non-finite input is not
    supported (the scale of such a row is not finite).  Not differentiable."""
    if not isinstance(x, Tensor):
        raise TypeError('x must be a Tensor')
    if x.dim() != 2:
        raise ValueError('quantize_rows: x must be [N, F], got %d dimensions' % x.dim())
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError('quantize_rows: float32, bfloat16 or float16 expected, got %s' % x.dtype)
    xq, scale = torch.ops.tsamd.quantize_rows(x)
    return xq, scale


def matmul_q8(src: SparseTensor, xq: Tensor, scale: Optional[Tensor] = None, reduce: str = 'sum',
              out_dtype: torch.dtype = torch.float32) -> Tensor:
    """``out[i, :] = reduce over the entries e of row i of value[e] * scale[col[e]] * decode(xq[col[e], :])``:
    ``xq [N, F]`` in ``torch.float8_e4m3fn`` (``F <= 1024``, at any storage offset), ``scale [N]`` float32 or ``None``
    (ones) -> ``[M, F]`` in ``out_dtype`` (float32 or bfloat16).  ``reduce`` is ``'sum'`` (``'add'``) or ``'mean'``
    (divided by the number of entries, as ``matmul``); a row without entries gives 0.  float32 accumulation, one rounding
    on the store; deterministic.  Values are ``None`` or one weight per entry (bfloat16 / float16 values are converted
    to float32).  Not differentiable: the features are constants, and values that require a gradient are refused."""
    if not isinstance(xq, Tensor):
        raise TypeError('xq must be a Tensor')
    if xq.dtype != torch.float8_e4m3fn:
        raise TypeError('matmul_q8: xq must be torch.float8_e4m3fn, got %s (quantize_rows makes it)' % xq.dtype)
    if xq.dim() != 2:
        raise ValueError('matmul_q8: xq must be [N, F], got %d dimensions (a batched x is not supported)' % xq.dim())
    if xq.size(0) != src.sparse_size(1):
        raise ValueError('xq has %d rows, the sparse pattern has %d columns' % (xq.size(0), src.sparse_size(1)))
    if xq.size(1) > _MAX_F:
        raise ValueError('matmul_q8: F must be at most %d, got %d' % (_MAX_F, xq.size(1)))
    if reduce == 'add':
        reduce = 'sum'
    if reduce not in ('sum', 'mean'):
        raise ValueError("matmul_q8: reduce must be 'sum' or 'mean', got %r" % (reduce, ))
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError('matmul_q8: out_dtype must be torch.float32 or torch.bfloat16, got %s' % (out_dtype, ))
    if scale is not None:
        if not isinstance(scale, Tensor) or scale.dtype != torch.float32:
            raise TypeError('matmul_q8: scale must be a float32 Tensor')
        if scale.dim() != 1 or scale.size(0) != xq.size(0):
            raise ValueError('matmul_q8: scale must be [%d], got %s' % (xq.size(0), tuple(scale.shape)))
        scale = scale.detach()
    st = src.storage
    value = st.value()
    if value is not None:
        if value.dim() != 1:
            raise ValueError('matmul_q8 needs one weight per entry, got values of shape %s' % (tuple(value.shape), ))
        if value.requires_grad and torch.is_grad_enabled():
            raise ValueError('matmul_q8: values that require a gradient are not supported; detach them')
        if not value.is_floating_point() or value.dtype == torch.float64:
            raise TypeError('matmul_q8: values must be float32, bfloat16 or float16, got %s' % value.dtype)
        value = value.detach().to(torch.float32)
    return torch.ops.tsamd.spmm_q8(st.rowptr(), st.col(), value, xq, scale, reduce, out_dtype == torch.bfloat16)


SparseTensor.matmul_q8 = (lambda self, xq, scale=None, reduce='sum', out_dtype=torch.float32:
                          matmul_q8(self, xq, scale, reduce, out_dtype))
