"""Fused multi-aggregation: several reductions of ``A @ x`` in one gather of ``x`` (csrc/spmm_multi.hip).

What PNA (``mean``, ``min``, ``max``, ``std``), PyG's ``MultiAggregation`` and ``SAGEConv(aggr=[...])`` ask of one
adjacency: today one ``matmul`` per reduction, each paying for the random gather of ``x[col]`` again, and ``var`` /
``std`` built by hand from ``A @ x`` and ``A @ x**2``.
"""
from typing import List, Sequence

import torch
from torch import Tensor

from .tensor import SparseTensor

# bit of every reduction in the operator's mask (tsamd_multi in include/tsamd.h); the slots of the operator's output
# are in this order
_BITS = {'sum': 1, 'mean': 2, 'min': 4, 'max': 8, 'var': 16, 'std': 32}


def _reductions(reduce: Sequence[str]) -> List[str]:
    if isinstance(reduce, str) or len(reduce) == 0:
        raise ValueError("reduce must be a non-empty list drawn from 'sum', 'mean', 'min', 'max', 'var', 'std'")
    names = ['sum' if r == 'add' else r for r in reduce]
    for r in names:
        if r not in _BITS:
            raise ValueError("unknown reduce %r: expected 'sum', 'mean', 'min', 'max', 'var' or 'std'" % (r, ))
    if len(set(names)) != len(names):
        raise ValueError('a reduction may be given once, got %s' % (list(reduce), ))
    return names


def matmul_multi(src: SparseTensor, x: Tensor, reduce: Sequence[str]) -> Tensor:
    """``out[:, i] = reduce[i]`` over the products ``value[e] * x[col[e], :]`` of every row, for a list ``reduce`` drawn
    from ``'sum'`` (``'add'``), ``'mean'``, ``'min'``, ``'max'``, ``'var'`` and ``'std'``: ``x [N, F]`` -> ``[M, R, F]``
    in the dtype of ``x``, so that ``out.flatten(1)`` is the concatenation ``MultiAggregation(mode='cat')`` produces.
    ``sum``, ``mean``, ``min`` and ``max`` are those of ``matmul``; ``var`` is the population variance of the row's
    products (never negative, not computed as ``E[y^2] - E[y]^2``) and ``std`` its root; a row without entries gives 0.
    All reductions share one gather of ``x``.  Differentiable (once) with respect to ``x``; a batched ``x`` and values
    that require a gradient are refused."""
    names = _reductions(reduce)
    if not isinstance(x, Tensor):
        raise TypeError('x must be a Tensor')
    if x.dim() != 2:
        raise ValueError('matmul_multi: x must be [N, F], got %d dimensions (a batched x is not supported)' % x.dim())
    if not x.is_floating_point():
        raise ValueError('matmul_multi: x must be floating point, got %s' % x.dtype)
    if x.size(0) != src.sparse_size(1):
        raise ValueError('x has %d rows, the sparse pattern has %d columns' % (x.size(0), src.sparse_size(1)))
    st = src.storage
    value = st.value()
    if value is not None:
        if value.dim() != 1:
            raise ValueError('matmul_multi needs one weight per entry, got values of shape %s' % (tuple(value.shape), ))
        if value.requires_grad and torch.is_grad_enabled():
            raise ValueError('matmul_multi: values that require a gradient are not supported; detach them, or call '
                             'matmul once per reduction')
        value = value.detach().to(x.dtype)
    mask = 0
    for r in names:
        mask |= _BITS[r]
    colptr = csr2csc = row = None
    if x.requires_grad and torch.is_grad_enabled():  # the CSC side is built only for a backward, as in storage_spmm
        colptr, csr2csc, row = st.colptr(), st.csr2csc(), st.row()
    out = torch.ops.tsamd.spmm_multi(st.rowptr(), st.col(), value, colptr, csr2csc, row, x, mask)[0]
    order = sorted(names, key=_BITS.get)
    if order == names:
        return out
    return out[:, [order.index(r) for r in names]]


SparseTensor.matmul_multi = lambda self, x, reduce: matmul_multi(self, x, reduce)
