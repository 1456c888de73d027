"""Row / column softmax over the stored entries of a SparseTensor: the normalisation of attention layers
("a score per edge, softmax over the neighbours, aggregate"), ready for ``matmul``.

``dim = 1``: every row, segments from ``rowptr``; ``dim = 0``: every column, the values read through ``csr2csc`` and
segmented over ``colptr`` -- both one call of ``tsamd::segment_softmax`` (csrc/softmax.hip), which writes the result in
storage order.  ``dim = -1`` / ``-2`` name the rows / columns too.  ``dim >= 2`` is a plain softmax over a trailing value
dimension.  Trailing value dimensions are independent heads.  Differentiable w.r.t. the values (segment.py).
"""
import torch

from .segment import segment_softmax
from .tensor import SparseTensor


def softmax(src: SparseTensor, dim: int = 1) -> SparseTensor:
    if dim in (-1, -2):  # the sparse dimensions, whatever the shape of the values: -1 rows, -2 columns
        dim += 2
    if dim < 0 or dim >= src.dim():
        raise IndexError('dim out of range for a SparseTensor of %d dimensions' % src.dim())
    st = src.storage
    value = st.value()
    if value is not None and not value.is_floating_point():
        raise ValueError('softmax needs floating-point values, got %s' % value.dtype)
    if dim > 1:
        return src.set_value(torch.softmax(value, dim - 1), layout='coo')
    if value is None:  # all logits equal: 1 / count
        count, index = (st.rowcount(), st.row()) if dim == 1 else (st.colcount(), st.col())
        return src.set_value(count.to(torch.float32).reciprocal().index_select(0, index), layout='coo')
    if dim == 1:
        out = segment_softmax(value, None, st.rowptr(), src.size(0))
    else:
        out = segment_softmax(value, st.csr2csc(), st.colptr(), src.size(1))
    return src.set_value(out, layout='coo')


SparseTensor.softmax = lambda self, dim=1: softmax(self, dim)
