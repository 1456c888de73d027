"""Attention over a sparse pattern: the two ends of ``scores -> softmax -> aggregate``, and the three fused.

``sddmm(adj, q, k, scale)``   a score per stored entry and head, ``scale * <q[row], k[col]>``, as the values of ``adj``
                              (``tsamd::sddmm_heads``, csrc/sddmm.hip) -- no ``[nnz, H, D]`` gather is materialised;
``matmul_heads(adj, x)``      ``out[m, h] = sum_n adj[m, n, h] * x[n, h]`` for ``[nnz, H]`` values
                              (``tsamd::spmm_heads``, csrc/spmm_heads.hip) -- no Python loop over the heads.

With ``SparseTensor.softmax`` in between::

    out = adj.sddmm(q, k, D ** -0.5).softmax(1).matmul_heads(v)

Both are differentiable (once), and the two kernels close over each other: the gradient of ``sddmm`` w.r.t. ``q`` is
the multi-head SpMM with the score gradient as values, w.r.t. ``k`` the same on the columns (``colptr``, ``csr2csc``);
the value gradient of ``matmul_heads`` is an SDDMM of ``grad_out`` with ``x``, its ``x`` gradient the SpMM on the columns.
The column-side caches of the storage are only built when such a gradient will be asked for.

``attention(adj, q, k, v, scale=None, bias=False, dropout=0.0, training=True, seed=None)`` is the whole chain in one call (``tsamd::attention_heads``,
csrc/attention.hip): the scores are formed, normalised with an online softmax over the row and multiplied into ``v``
in one pass over the entries, so the forward writes nothing of size ``nnz``.  It keeps ``out`` and the row-wise
``lse = log sum exp(score)`` for the backward, where one kernel (``tsamd::attention_heads_bw``) recomputes the
probabilities ``p`` and the score gradients ``ds = p * (<grad_out, v> - <grad_out, out>)`` per entry and
``tsamd::spmm_heads`` turns them into ``grad_q``, ``grad_k`` and ``grad_v``; ``ds`` itself is the gradient of the bias.

``gat_attention(adj, a_dst, a_src, v, negative_slope=0.2, bias=False, dropout=0.0, training=True, seed=None)`` is the same fused pass for the additive score
of a graph attention network (``tsamd::gat_attention_heads``): ``leaky_relu(a_dst[row] + a_src[col] (+ the edge
term))`` with one scalar per node and head, so no ``[nnz, H]`` gather, add, activation or softmax array is written.
Its backward kernel (``tsamd::gat_attention_heads_bw``) gives ``p`` and ``dz``, the gradient of the pre-activation;
``tsamd::segment_reduce`` sums ``dz`` over the rows into ``grad_a_dst`` and over the columns into ``grad_a_src``.

Both fused calls take ``dropout`` on the probabilities (the DROP instantiations of the same kernels): the mask is a
Philox function of ``(seed, entry, head)`` recomputed in the backward, so training with attention dropout keeps the
fused pass and its memory: ``out = sum softmax(score) * keep / (1 - dropout) * v``, and the backward kernel returns
``p * keep / (1 - dropout)`` and ``ds = p * (keep / (1 - dropout) * <grad_out, v> - <grad_out, out>)``.
"""
from typing import Optional

import torch
from torch import Tensor

from .tensor import SparseTensor


def _csc_side(st):
    """(colptr, row ids in column order, csr2csc): the segmented order of the columns"""
    csr2csc = st.csr2csc()
    return st.colptr(), st.row().index_select(0, csr2csc), csr2csc


class _SddmmHeads(torch.autograd.Function):
    """scores = tsamd::sddmm_heads; grad_q = scale * spmm_heads(rows; g, k), grad_k = scale * spmm_heads(columns; g, q)"""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, row: Optional[Tensor], rowptr: Tensor, col: Tensor,
                colptr: Optional[Tensor], row_csc: Optional[Tensor], csr2csc: Optional[Tensor], scale: float):
        out = torch.ops.tsamd.sddmm_heads(row, rowptr, col, None, q.detach(), k.detach(), scale)
        ctx.scale = scale
        ctx.has_csc = colptr is not None
        ctx.save_for_backward(*([q, k, rowptr, col] + ([colptr, row_csc, csr2csc] if ctx.has_csc else [])))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out: Tensor):
        q, k, rowptr, col = ctx.saved_tensors[:4]
        g = grad_out.contiguous()
        grad_q = grad_k = None
        if ctx.needs_input_grad[0]:
            grad_q = torch.ops.tsamd.spmm_heads(rowptr, col, None, g, k, q.size(0))
            if ctx.scale != 1.0:
                grad_q.mul_(ctx.scale)
        if ctx.needs_input_grad[1]:
            colptr, row_csc, csr2csc = ctx.saved_tensors[4:7]
            grad_k = torch.ops.tsamd.spmm_heads(colptr, row_csc, csr2csc, g, q, k.size(0))
            if ctx.scale != 1.0:
                grad_k.mul_(ctx.scale)
        return grad_q, grad_k, None, None, None, None, None, None, None


class _SpmmHeads(torch.autograd.Function):
    """out = tsamd::spmm_heads; grad_value = sddmm_heads(grad_out, x), grad_x = spmm_heads(columns; value, grad_out)"""

    @staticmethod
    def forward(ctx, value: Tensor, x: Tensor, row: Optional[Tensor], rowptr: Tensor, col: Tensor,
                colptr: Optional[Tensor], row_csc: Optional[Tensor], csr2csc: Optional[Tensor], nseg: int):
        out = torch.ops.tsamd.spmm_heads(rowptr, col, None, value.detach(), x.detach(), nseg)
        ctx.has_row = row is not None
        ctx.has_csc = colptr is not None
        ctx.save_for_backward(*([value, x, rowptr, col] + ([row] if ctx.has_row else []) +
                                ([colptr, row_csc, csr2csc] if ctx.has_csc else [])))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out: Tensor):
        value, x, rowptr, col = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        row = rest.pop(0) if ctx.has_row else None
        g = grad_out.contiguous()  # expanded / transposed gradients arrive here
        grad_value = grad_x = None
        if ctx.needs_input_grad[0]:
            grad_value = torch.ops.tsamd.sddmm_heads(row, rowptr, col, None, g, x, 1.0)
        if ctx.needs_input_grad[1]:
            colptr, row_csc, csr2csc = rest
            grad_x = torch.ops.tsamd.spmm_heads(colptr, row_csc, csr2csc, value, g, x.size(0))
        return grad_value, grad_x, None, None, None, None, None, None, None


# ---- the fused calls.  Dot-product and additive scores share the bookkeeping of their autograd pair; below, (sr, sc)
# are the score operands of the rows and of the columns, (q, k) or (a_dst, a_src), and `scalar` is scale or negative_slope
def _fused_forward(ctx, op: str, sr: Tensor, sc: Tensor, v: Tensor, bias: Optional[Tensor], row: Optional[Tensor],
                   rowptr: Tensor, col: Tensor, colptr: Optional[Tensor], row_csc: Optional[Tensor],
                   csr2csc: Optional[Tensor], scalar: float, dropout: float = 0.0, seed: int = 0) -> Tensor:
    """out of ``tsamd::<op>``; saves (operands, out, lse, rowptr, col, [bias], [row], [colptr, row_csc, csr2csc]) and keeps
    (dropout, seed): the backward recomputes the mask"""
    b = None if bias is None else bias.detach()
    out, lse = getattr(torch.ops.tsamd, op)(rowptr, col, b, sr.detach(), sc.detach(), v.detach(), scalar, dropout, seed)
    ctx.scalar, ctx.dropout, ctx.seed = scalar, dropout, seed
    ctx.has_bias, ctx.has_row, ctx.has_csc = bias is not None, row is not None, colptr is not None
    ctx.save_for_backward(*([sr, sc, v, out, lse, rowptr, col] + ([bias] if ctx.has_bias else []) +
                            ([row] if ctx.has_row else []) + ([colptr, row_csc, csr2csc] if ctx.has_csc else [])))
    return out


def _fused_backward(ctx, op_bw: str, grad_out: Tensor):
    """(p, d) = ``tsamd::<op_bw>`` on what the forward saved -> (sr, sc, d, rowptr, col, the column side or None, grad_v,
    grad_bias): grad_v = spmm_heads(columns; p, grad_out), grad_bias = d, summed over the heads for a [nnz] bias.  The
    gradients of the score operands are the caller's.  With dropout the kernel gives ``p * keep * c`` for p and
    ``d = p * (keep * c * <grad_out, v> - <grad_out, out>)``: nothing else changes here."""
    sr, sc, v, out, lse, rowptr, col = ctx.saved_tensors[:7]
    rest = list(ctx.saved_tensors[7:])
    bias = rest.pop(0) if ctx.has_bias else None
    row = rest.pop(0) if ctx.has_row else None
    csc = rest if ctx.has_csc else None
    g = grad_out.contiguous()  # expanded / transposed gradients arrive here
    p, d = getattr(torch.ops.tsamd, op_bw)(row, rowptr, col, bias, sr, sc, v, out, lse, g, ctx.scalar, ctx.dropout,
                                           ctx.seed)
    grad_v = grad_bias = None
    if ctx.needs_input_grad[2]:
        grad_v = torch.ops.tsamd.spmm_heads(csc[0], csc[1], csc[2], p, g, v.size(0))
    if ctx.has_bias and ctx.needs_input_grad[3]:
        grad_bias = d if bias.dim() == 2 else d.sum(1, dtype=lse.dtype).to(d.dtype)
    return sr, sc, d, rowptr, col, csc, grad_v, grad_bias


class _AttentionHeads(torch.autograd.Function):
    """out = tsamd::attention_heads; backward: (p, ds) = tsamd::attention_heads_bw, then grad_q = scale * spmm_heads(rows;
    ds, k), grad_k = scale * spmm_heads(columns; ds, q), grad_v = spmm_heads(columns; p, grad_out), grad_bias = ds"""

    @staticmethod
    def forward(ctx, q: Tensor, k: Tensor, v: Tensor, *bias_pattern_scale_dropout):
        return _fused_forward(ctx, 'attention_heads', q, k, v, *bias_pattern_scale_dropout)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out: Tensor):
        q, k, ds, rowptr, col, csc, grad_v, grad_bias = _fused_backward(ctx, 'attention_heads_bw', grad_out)
        grad_q = grad_k = None
        if ctx.needs_input_grad[0]:
            grad_q = torch.ops.tsamd.spmm_heads(rowptr, col, None, ds, k, q.size(0))
            if ctx.scalar != 1.0:
                grad_q.mul_(ctx.scalar)
        if ctx.needs_input_grad[1]:
            grad_k = torch.ops.tsamd.spmm_heads(csc[0], csc[1], csc[2], ds, q, k.size(0))
            if ctx.scalar != 1.0:
                grad_k.mul_(ctx.scalar)
        return grad_q, grad_k, grad_v, grad_bias, None, None, None, None, None, None, None, None, None


class _GatAttentionHeads(torch.autograd.Function):
    """out = tsamd::gat_attention_heads; backward: (p, dz) = tsamd::gat_attention_heads_bw, then grad_a_dst = the sum of dz
    over the rows, grad_a_src = the sum of dz over the columns (tsamd::segment_reduce), grad_v = spmm_heads(columns; p,
    grad_out), grad_bias = dz"""

    @staticmethod
    def forward(ctx, a_dst: Tensor, a_src: Tensor, v: Tensor, *bias_pattern_slope_dropout):
        return _fused_forward(ctx, 'gat_attention_heads', a_dst, a_src, v, *bias_pattern_slope_dropout)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out: Tensor):
        a_dst, a_src, dz, rowptr, col, csc, grad_v, grad_bias = _fused_backward(ctx, 'gat_attention_heads_bw', grad_out)
        grad_dst = grad_src = None
        if ctx.needs_input_grad[0]:
            grad_dst = torch.ops.tsamd.segment_reduce(dz, None, rowptr, a_dst.size(0), 'sum', True)
        if ctx.needs_input_grad[1]:
            grad_src = torch.ops.tsamd.segment_reduce(dz, csc[2], csc[0], a_src.size(0), 'sum', True)
        return grad_dst, grad_src, grad_v, grad_bias, None, None, None, None, None, None, None, None, None


def _fused(adj: SparseTensor, fn, op: str, sr: Tensor, sc: Tensor, v: Tensor, b: Optional[Tensor],
           scalar: float, dropout: float = 0.0, seed: int = 0) -> Tensor:
    """The fused call: through the autograd pair `fn` where a gradient will be asked for -- with the column side of the
    pattern when it is sc's or v's -- and through ``tsamd::<op>`` alone where none will.  ``dropout == 0`` passes neither
    the rate nor a seed: the call as it was before dropout existed"""
    extra = (dropout, seed) if dropout != 0.0 else ()
    st = adj.storage
    rowptr, col = st.rowptr(), st.col()
    grad = torch.is_grad_enabled()
    if grad and (sr.requires_grad or sc.requires_grad or v.requires_grad or (b is not None and b.requires_grad)):
        csc = _csc_side(st) if sc.requires_grad or v.requires_grad else (None, None, None)
        return fn.apply(sr, sc, v, b, st._row, rowptr, col, csc[0], csc[1], csc[2], scalar, *extra)
    return getattr(torch.ops.tsamd, op)(rowptr, col, b, sr, sc, v, scalar, *extra)[0]


def _host_seed() -> int:
    """One seed in [0, 2^63 - 1) from torch's CPU generator -- ``host_seed()`` of csrc/ops_sample.h, the samplers' rule:
    reproducible under ``torch.manual_seed``, a new one per call, no device sync"""
    return int(torch.randint(0, torch.iinfo(torch.int64).max, (1, ), dtype=torch.long))


def _dropout_args(dropout, training: bool, seed):
    """(rate, seed) of a fused call: (0.0, 0) where nothing is dropped"""
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)):
        raise TypeError('dropout must be a float, got %s' % type(dropout).__name__)
    dropout = float(dropout)
    if not 0.0 <= dropout < 1.0:  # NaN fails both comparisons
        raise ValueError('dropout must be a rate in [0, 1), got %r' % dropout)
    if seed is not None:
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError('seed must be an int or None, got %s' % type(seed).__name__)
        if not 0 <= seed < 2 ** 63:
            raise ValueError('seed must be in [0, 2^63), got %d' % seed)
    if dropout == 0.0 or not training:
        return 0.0, 0
    return dropout, _host_seed() if seed is None else seed


def _edge_bias(adj: SparseTensor, H: int, dtype: torch.dtype, who: str) -> Tensor:
    """The values of ``adj`` as the bias of a fused call with ``H`` heads, in ``dtype``; ``who`` is the operand the message
    counts the heads of"""
    b = adj.storage.value()
    if b is None:
        raise ValueError('bias=True needs a SparseTensor with values, this one has none')
    if not b.is_floating_point():
        raise ValueError('the bias must be floating point, got %s values' % b.dtype)
    if b.dim() not in (1, 2) or (b.dim() == 2 and b.size(1) != H):
        raise ValueError('the bias must be [nnz] or [nnz, %d] values (%s has %d heads), got %s'
                         % (H, who, H, tuple(b.shape)))
    return b.to(dtype)


def _check_operand(t: Tensor, name: str, rows: int, what: str) -> None:
    if not isinstance(t, Tensor):
        raise TypeError('%s must be a Tensor' % name)
    if not t.is_floating_point():
        raise ValueError('%s must be floating point, got %s' % (name, t.dtype))
    if t.size(0) != rows:
        raise ValueError('%s has %d rows, the sparse pattern has %d %s' % (name, t.size(0), rows, what))


def sddmm(adj: SparseTensor, q: Tensor, k: Tensor, scale: float = 1.0) -> SparseTensor:
    """``adj`` with the values ``scale * (q[row] * k[col]).sum(-1)``: ``[nnz]`` for ``q [M, D]``, ``k [N, D]``, ``[nnz, H]``
    for ``q [M, H, D]``, ``k [N, H, D]``, in storage order.  Only the pattern of ``adj`` is used, its values are not
    read.  Differentiable (once) w.r.t. ``q`` and ``k``."""
    if q.dim() != k.dim() or q.dim() not in (2, 3):
        raise ValueError('q and k must both be [rows, D] or [rows, H, D], got %d and %d dimensions'
                         % (q.dim(), k.dim()))
    _check_operand(q, 'q', adj.sparse_size(0), 'rows')
    _check_operand(k, 'k', adj.sparse_size(1), 'columns')
    if q.dtype != k.dtype:
        raise ValueError('q and k differ in dtype: %s and %s' % (q.dtype, k.dtype))
    if q.shape[1:] != k.shape[1:]:
        raise ValueError('q is %s per row, k is %s: heads and features must agree'
                         % (tuple(q.shape[1:]), tuple(k.shape[1:])))
    flat = q.dim() == 2
    if flat:
        q, k = q.unsqueeze(1), k.unsqueeze(1)
    st = adj.storage
    rowptr, col, row = st.rowptr(), st.col(), st._row
    grad = torch.is_grad_enabled()
    if grad and (q.requires_grad or k.requires_grad):
        colptr, row_csc, csr2csc = _csc_side(st) if k.requires_grad else (None, None, None)
        out = _SddmmHeads.apply(q, k, row, rowptr, col, colptr, row_csc, csr2csc, float(scale))
    else:
        out = torch.ops.tsamd.sddmm_heads(row, rowptr, col, None, q, k, float(scale))
    return adj.set_value(out.squeeze(1) if flat else out, layout='coo')


def matmul_heads(adj: SparseTensor, x: Tensor) -> Tensor:
    """``out[m, h, :] = sum over the stored entries (m, n) of value[(m, n), h] * x[n, h, :]``: values ``[nnz, H]``,
    ``x [N, H, D]`` -> ``[M, H, D]``; rows without entries are zeros.  Differentiable (once) w.r.t. the values and
    ``x``.  One weight per entry for all features is ``matmul``."""
    value = adj.storage.value()
    if value is None or value.dim() != 2:
        raise ValueError('matmul_heads needs [nnz, H] values, got %s; a SparseTensor without values or with one '
                         'weight per entry goes through matmul' % ('none' if value is None else tuple(value.shape)))
    if x.dim() != 3:
        raise ValueError('x must be [N, H, D], got %d dimensions' % x.dim())
    _check_operand(x, 'x', adj.sparse_size(1), 'columns')
    if not value.is_floating_point():
        raise ValueError('matmul_heads needs floating-point values, got %s' % value.dtype)
    if value.size(1) != x.size(1):
        raise ValueError('the values have %d heads, x has %d' % (value.size(1), x.size(1)))
    value = value.to(x.dtype)
    st = adj.storage
    rowptr, col, nseg = st.rowptr(), st.col(), adj.sparse_size(0)
    grad = torch.is_grad_enabled()
    if grad and (value.requires_grad or x.requires_grad):
        colptr, row_csc, csr2csc = _csc_side(st) if x.requires_grad else (None, None, None)
        return _SpmmHeads.apply(value, x, st._row, rowptr, col, colptr, row_csc, csr2csc, nseg)
    return torch.ops.tsamd.spmm_heads(rowptr, col, None, value, x, nseg)


def attention(adj: SparseTensor, q: Tensor, k: Tensor, v: Tensor, scale: Optional[float] = None,
              bias: bool = False, dropout: float = 0.0, training: bool = True, seed: Optional[int] = None) -> Tensor:
    """Attention over the pattern of ``adj`` in one fused pass: for row ``m`` and head ``h`` the score of a stored entry
    ``(m, n)`` is ``scale * <q[m, h], k[n, h]>`` (``scale=None``: ``D ** -0.5``), plus, with ``bias=True``, the entry's own
    value (``[nnz]`` shared by the heads or ``[nnz, H]``; ``-inf`` masks an entry); ``out[m, h] = sum_n softmax_n(score) *
    v[n, h]``.  ``q [M, H, D]``, ``k`` and ``v [N, H, D]`` -> ``[M, H, D]``; 2-D operands mean one head.  Rows without
    entries are zeros.  Differentiable (once) w.r.t. ``q``, ``k``, ``v`` and, with ``bias=True``, the values.

    ``dropout`` in ``[0, 1)`` drops each probability (per stored entry and head) with that rate and scales the kept ones by
    ``1 / (1 - dropout)``, as ``F.dropout`` on the ``[nnz, H]`` softmax output of the chain does; the softmax itself is not
    renormalised.  The mask is a counter-based function of ``(seed, entry, head)`` that forward and backward recompute, so
    still nothing of size ``nnz`` is kept.  ``training=False`` or ``dropout=0`` is the call without dropout, bit for bit.
    ``seed=None`` draws a seed from torch's CPU generator (reproducible under ``torch.manual_seed``, a new mask per call,
    no device sync); an int in ``[0, 2^63)`` fixes the mask."""
    dropout, seed = _dropout_args(dropout, training, seed)
    for t, name in ((q, 'q'), (k, 'k'), (v, 'v')):
        if not isinstance(t, Tensor):
            raise TypeError('%s must be a Tensor' % name)
    if not (q.dim() == k.dim() == v.dim()) or q.dim() not in (2, 3):
        raise ValueError('q, k and v must all be [rows, D] or [rows, H, D], got %d, %d and %d dimensions'
                         % (q.dim(), k.dim(), v.dim()))
    _check_operand(q, 'q', adj.sparse_size(0), 'rows')
    _check_operand(k, 'k', adj.sparse_size(1), 'columns')
    _check_operand(v, 'v', adj.sparse_size(1), 'columns')
    if q.dtype != k.dtype or q.dtype != v.dtype:
        raise ValueError('q, k and v differ in dtype: %s, %s and %s' % (q.dtype, k.dtype, v.dtype))
    if q.shape[1:] != k.shape[1:]:
        raise ValueError('q is %s per row, k is %s: heads and features must agree'
                         % (tuple(q.shape[1:]), tuple(k.shape[1:])))
    if v.shape != k.shape:
        raise ValueError('v must have the shape of k, got %s and %s: a value width of its own is not supported'
                         % (tuple(v.shape), tuple(k.shape)))
    flat = q.dim() == 2
    if flat:
        q, k, v = q.unsqueeze(1), k.unsqueeze(1), v.unsqueeze(1)
    H, D = q.size(1), q.size(2)
    if D == 0:
        raise ValueError('attention needs at least one feature per head')
    b = _edge_bias(adj, H, q.dtype, 'q') if bias else None
    scale = float(D) ** -0.5 if scale is None else float(scale)
    out = _fused(adj, _AttentionHeads, 'attention_heads', q, k, v, b, scale, dropout, seed)
    return out.squeeze(1) if flat else out


def gat_attention(adj: SparseTensor, a_dst: Tensor, a_src: Tensor, v: Tensor, negative_slope: float = 0.2,
                  bias: bool = False, dropout: float = 0.0, training: bool = True, seed: Optional[int] = None) -> Tensor:
    """Additive (graph attention network) attention over the pattern of ``adj`` in one fused pass: for row ``m`` and head
    ``h`` the score of a stored entry ``(m, n)`` is ``leaky_relu(a_dst[m, h] + a_src[n, h] + b, negative_slope)``, where
    ``b`` is, with ``bias=True``, the entry's own value (``[nnz]`` shared by the heads or ``[nnz, H]``) and zero without;
    ``out[m, h] = sum_n softmax_n(score) * v[n, h]``.  ``a_dst [M, H]``, ``a_src [N, H]``, ``v [N, H, D]`` -> ``[M, H, D]``;
    1-D ``a_dst`` / ``a_src`` with a 2-D ``v`` mean one head.  Rows without entries are zeros.

    The bias goes INSIDE the activation, where ``GATConv`` puts its edge term -- unlike the bias of ``attention``, which
    is added to the finished score.  So a ``-inf`` value masks its entry only for ``negative_slope > 0``: with a slope
    of ``0`` the product ``0 * -inf`` is NaN (IEEE) and the row is NaN; this is not special-cased.

    Differentiable (once) w.r.t. ``a_dst``, ``a_src``, ``v`` and, with ``bias=True``, the values; the derivative of the
    activation at ``z == 0`` is ``negative_slope``, as torch has it.

    ``dropout``, ``training`` and ``seed`` are those of ``attention``: dropout on the attention coefficients (``GATConv``'s
    ``dropout``), applied to the probabilities inside the fused pass."""
    dropout, seed = _dropout_args(dropout, training, seed)
    for t, name in ((a_dst, 'a_dst'), (a_src, 'a_src'), (v, 'v')):
        if not isinstance(t, Tensor):
            raise TypeError('%s must be a Tensor' % name)
    if not (a_dst.dim() == a_src.dim() == v.dim() - 1) or v.dim() not in (2, 3):
        raise ValueError('a_dst, a_src and v must be [rows], [columns] and [columns, D] or [rows, H], [columns, H] and '
                         '[columns, H, D], got %d, %d and %d dimensions' % (a_dst.dim(), a_src.dim(), v.dim()))
    _check_operand(a_dst, 'a_dst', adj.sparse_size(0), 'rows')
    _check_operand(a_src, 'a_src', adj.sparse_size(1), 'columns')
    _check_operand(v, 'v', adj.sparse_size(1), 'columns')
    if a_dst.dtype != a_src.dtype or a_dst.dtype != v.dtype:
        raise ValueError('a_dst, a_src and v differ in dtype: %s, %s and %s' % (a_dst.dtype, a_src.dtype, v.dtype))
    flat = v.dim() == 2
    if flat:
        a_dst, a_src, v = a_dst.unsqueeze(1), a_src.unsqueeze(1), v.unsqueeze(1)
    H, D = v.size(1), v.size(2)
    if a_dst.size(1) != H or a_src.size(1) != H:
        raise ValueError('a_dst has %d heads, a_src has %d, v has %d: the heads must agree'
                         % (a_dst.size(1), a_src.size(1), H))
    if D == 0:
        raise ValueError('gat_attention needs at least one feature per head')
    negative_slope = float(negative_slope)
    if negative_slope != negative_slope or negative_slope in (float('inf'), float('-inf')):
        raise ValueError('negative_slope must be finite, got %r' % negative_slope)
    b = _edge_bias(adj, H, v.dtype, 'v') if bias else None
    out = _fused(adj, _GatAttentionHeads, 'gat_attention_heads', a_dst, a_src, v, b, negative_slope, dropout, seed)
    return out.squeeze(1) if flat else out


SparseTensor.gat_attention = (lambda self, a_dst, a_src, v, negative_slope=0.2, bias=False, dropout=0.0, training=True,
                              seed=None: gat_attention(self, a_dst, a_src, v, negative_slope, bias, dropout, training, seed))
SparseTensor.attention = (lambda self, q, k, v, scale=None, bias=False, dropout=0.0, training=True, seed=None:
                          attention(self, q, k, v, scale, bias, dropout, training, seed))
SparseTensor.sddmm = lambda self, q, k, scale=1.0: sddmm(self, q, k, scale)
SparseTensor.matmul_heads = lambda self, x: matmul_heads(self, x)
