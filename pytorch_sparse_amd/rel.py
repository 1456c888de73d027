"""Relational (typed-edge) SpMM: one weight block per relation, contracted on the matrix instructions
(csrc/rel_gemm.hip, csrc/ops_rel.cpp).

What R-GCN and the message step of every heterogeneous layer compute over a typed adjacency -- today a Python loop over
the relations of ``masked_select_nnz``, ``matmul`` and ``x @ W[r]``.
"""
from typing import Optional

import torch
from torch import Tensor

from .tensor import SparseTensor


def matmul_rel(src: SparseTensor, x: Tensor, weight: Tensor, rel: Tensor, reduce: str = 'sum') -> Tensor:
    """``out[i, :] = sum over the entries e of row i of value[e] * (x[col[e], :] @ weight[rel[e]])``: ``x [N, F]``,
    ``weight [R, F, Fo]`` in the dtype of ``x`` (float32 or bfloat16, ``F`` and ``Fo`` in ``1 .. 512``), ``rel`` an int64
    ``[nnz]`` tensor in the order of ``src.storage.col()`` with values in ``[0, R)`` -> ``[M, Fo]`` in the dtype of
    ``x``.  ``reduce='mean'`` is R-GCN's default: the sum over the relations of the mean over the entries of every
    (row, relation) pair.  fp32 accumulation; deterministic.  Differentiable (once) with respect to ``x`` and
    ``weight``; a batched ``x`` and values that require a gradient are refused.  Scriptable.

    A 4-D ``weight [R, B, ci, co]`` (``B * ci = F``, ``Fo = B * co``) is R-GCN's block-diagonal decomposition,
    ``weight[r] = diag(weight[r, 0] .. weight[r, B - 1])``: ``out[i, b co + n] = sum_e value[e] sum_k x[col[e], b ci + k]
    weight[rel[e], b, k, n]``, contracted block by block (csrc/rel_blocks.hip); its gradient is ``[R, B, ci, co]``."""
    if reduce == 'add':
        reduce = 'sum'
    if reduce != 'sum' and reduce != 'mean':
        raise ValueError("matmul_rel: reduce must be 'sum' or 'mean'")
    if x.dim() != 2:
        raise ValueError('matmul_rel: x must be [N, F], got %d dimensions (a batched x is not supported)' % x.dim())
    if x.dtype != torch.float32 and x.dtype != torch.bfloat16:
        raise ValueError('matmul_rel: float32 or bfloat16 expected (float16 and float64 are not supported)')
    if x.size(0) != src.sparse_size(1):
        raise ValueError('x has %d rows, the sparse pattern has %d columns' % (x.size(0), src.sparse_size(1)))
    if weight.dim() == 4:
        if (weight.size(0) < 1 or weight.size(1) < 1 or weight.size(2) < 1 or weight.size(3) < 1
                or weight.size(1) * weight.size(2) != x.size(1)):
            raise ValueError('matmul_rel: a block-diagonal weight must be [R, B, ci, co] with R >= 1 and B * ci = %d, '
                             'got [%d, %d, %d, %d]' % (x.size(1), weight.size(0), weight.size(1), weight.size(2),
                                                       weight.size(3)))
        Fo = weight.size(1) * weight.size(3)
    else:
        if weight.dim() != 3:
            raise ValueError('matmul_rel: weight must be [R, F, Fo], got %d dimensions' % weight.dim())
        if weight.size(0) < 1 or weight.size(1) != x.size(1):
            raise ValueError('matmul_rel: weight must be [R, F, Fo] with R >= 1 and F = %d, got [%d, %d, %d]' %
                             (x.size(1), weight.size(0), weight.size(1), weight.size(2)))
        Fo = weight.size(2)
    if weight.dtype != x.dtype:
        raise ValueError('matmul_rel: weight and x differ in dtype')
    if x.size(1) < 1 or x.size(1) > 512 or Fo < 1 or Fo > 512:
        raise ValueError('matmul_rel: F and Fo must lie in 1 .. 512, got %d and %d' % (x.size(1), Fo))
    if rel.dtype != torch.int64 or rel.dim() != 1 or rel.numel() != src.nnz():
        raise ValueError('matmul_rel: rel must be an int64 tensor with one relation per entry ([%d]), got %d element(s) '
                         'in %d dimension(s)' % (src.nnz(), rel.numel(), rel.dim()))
    st = src.storage
    value = st.value()
    if value is not None:
        if value.dim() != 1:
            raise ValueError('matmul_rel needs one weight per entry, got values of %d dimensions' % value.dim())
        if value.requires_grad and torch.is_grad_enabled():
            raise ValueError('matmul_rel: values that require a gradient are not supported; detach them')
        value = value.detach().to(x.dtype)
    colptr: Optional[Tensor] = None
    csr2csc: Optional[Tensor] = None
    if x.requires_grad and torch.is_grad_enabled():  # the CSC side is built only for a backward, as in storage_spmm
        colptr = st.colptr()
        csr2csc = st.csr2csc()
    return torch.ops.tsamd.spmm_rel(st.rowptr(), st.col(), value, st.row(), rel, colptr, csr2csc, x, weight, reduce)


SparseTensor.matmul_rel = lambda self, x, weight, rel, reduce='sum': matmul_rel(self, x, weight, rel, reduce)
