"""fp64 reference of the sum / mean SpMM and of both its gradients, the comparator that goes with it, and the
graphs / widths the backward tests sweep.  Not collected by pytest; no kernel of the project is involved.

For a matrix in COO form ``(row, col, value or None)`` with ``M`` rows, ``x[..., N, K]`` and ``g[..., M, K]``, with
``deg = max(rowcount, 1)`` and ``w_e = value_e`` (or 1), divided by ``deg[row_e]`` for mean:

    out[b, m, :]      = sum_{e: row_e = m} w_e * x[b, col_e, :]
    grad_value[e]     = sum_b sum_k x[b, col_e, k] * g[b, row_e, k]      (/ deg[row_e] for mean)
    grad_mat[b, n, :] = sum_{e: col_e = n} w_e * g[b, row_e, :]

Beside each result stands its L1 mass (the same sum over absolute values); a floating result of dtype T is accepted when
``|got - exact| <= SUM_TOL[T] * L1 + SUM_ATOL[T]`` (tests/util.py).  The entries may come in any order and may repeat.
"""
from collections import namedtuple

import numpy as np
import torch

from tests.util import SUM_ATOL, SUM_TOL

Reference = namedtuple('Reference', 'out out_l1 grad_value grad_value_l1 grad_mat grad_mat_l1')
Graph = namedtuple('Graph', 'row col rowptr M N hub_row hub_col unreferenced')

VECTOR_SLOTS = (1, 2, 3, 4, 5, 8, 16, 24, 32, 33, 63, 64, 65, 96, 128, 130)
SCALAR_K = (1, 2, 3, 5, 7, 33, 63, 65, 129, 131)
FP16_MAX = 65504.0


# ---- the three formulas ---------------------------------------------------------------------------------------
def _deg(row, M):
    return torch.bincount(row, minlength=M).clamp(min=1).double()


def _weights(row, value, reduce, M):
    assert reduce in ('sum', 'mean')
    w = torch.ones(row.numel(), dtype=torch.float64) if value is None else value.detach().cpu().double()
    return w / _deg(row, M)[row] if reduce == 'mean' else w


def _batched(t, rows):
    t = t.detach().cpu().double()
    assert t.dim() >= 2 and t.size(-2) == rows
    return t.reshape(-1, rows, t.size(-1)), tuple(t.shape[:-2])


def _chunks(E, per_entry):
    """Entry ranges whose [B, chunk, K] temporaries stay near 2^24 elements (a large matrix is summed piecewise)."""
    step = max(1, (1 << 24) // max(per_entry, 1))
    return [(s, min(E, s + step)) for s in range(0, E, step)]


def _scatter_rows(src, gather, scatter, w, rows):
    """(sum, L1 mass) [B, rows, K] of w_e * src[:, gather_e, :] added into row scatter_e."""
    shape = (src.size(0), rows, src.size(2))
    tot, l1 = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    for s, e in _chunks(gather.numel(), src.size(0) * src.size(2)):
        prod = w[s:e].view(1, -1, 1) * src[:, gather[s:e], :]
        tot.index_add_(1, scatter[s:e], prod)
        l1.index_add_(1, scatter[s:e], prod.abs_())
    return tot, l1


def forward(row, col, value, x, reduce, M):
    """(out, L1 mass), both fp64 of shape [..., M, K]."""
    xb, batch = _batched(x, x.size(-2))
    out, l1 = _scatter_rows(xb, col, row, _weights(row, value, reduce, M), M)
    return out.reshape(*batch, M, -1), l1.reshape(*batch, M, -1)


def grad_value(row, col, x, g, reduce, M):
    """(grad_value, L1 mass), both fp64 of shape [E]."""
    xb, _ = _batched(x, x.size(-2))
    gb, _ = _batched(g, M)
    assert xb.size(0) == gb.size(0) and xb.size(2) == gb.size(2)
    assert reduce in ('sum', 'mean')
    E = row.numel()
    gv, l1 = torch.zeros(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    for s, e in _chunks(E, xb.size(0) * xb.size(2)):
        prod = xb[:, col[s:e], :] * gb[:, row[s:e], :]
        gv[s:e] = prod.sum((0, 2))
        l1[s:e] = prod.abs_().sum((0, 2))
    scale = 1.0 / _deg(row, M)[row] if reduce == 'mean' else torch.ones(E, dtype=torch.float64)
    return gv * scale, l1 * scale


def grad_mat(row, col, value, g, reduce, M, N):
    """(grad_mat, L1 mass), both fp64 of shape [..., N, K]."""
    gb, batch = _batched(g, M)
    gm, l1 = _scatter_rows(gb, row, col, _weights(row, value, reduce, M), N)
    return gm.reshape(*batch, N, -1), l1.reshape(*batch, N, -1)


def reference(row, col, value, x, g, reduce, M):
    row, col = row.cpu(), col.cpu()
    return Reference(*forward(row, col, value, x, reduce, M), *grad_value(row, col, x, g, reduce, M),
                     *grad_mat(row, col, value, g, reduce, M, x.size(-2)))


# ---- the comparator -------------------------------------------------------------------------------------------
def bound_ratio(got, exact, l1, dtype):
    """max over the elements of |got - exact| / (SUM_TOL * L1 + SUM_ATOL); inf when shapes differ or when `got` holds
    a value that is not finite where the exact one is (a NaN never passes)."""
    got = got.detach().cpu().double()
    if tuple(got.shape) != tuple(exact.shape):
        return float('inf')
    if got.numel() == 0:
        return 0.0
    err = (got - exact).abs()
    ratio = err / (SUM_TOL[dtype] * l1 + SUM_ATOL[dtype])
    ratio = torch.where(torch.isfinite(got) & torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    return float(ratio.max())


def assert_within_bound(got, exact, l1, dtype, what=''):
    r = bound_ratio(got, exact, l1, dtype)
    assert r <= 1.0, '%s: max |err| / bound = %.3g (%s)' % (what, r, dtype)
    return r


# ---- the plain same-precision computation (what the bound has to leave room for) --------------------------------
def plain_same_precision(row, col, value, x, g, reduce, M):
    """The three results computed the plain way in the working precision: products and sums in fp32 (fp64 for fp64)
    in entry order, one rounding to the dtype T of `x`; the mean weight of grad_mat is value / T(deg) (or 1 / T(deg))
    rounded to T, as the autograd glue forms it.  -> (out, grad_value, grad_mat) of dtype T."""
    T = x.dtype
    A = np.float64 if T == torch.float64 else np.float32
    tA = torch.float64 if T == torch.float64 else torch.float32
    row, col = row.cpu(), col.cpu()
    r, c = row.numpy(), col.numpy()
    N, K = x.size(-2), x.size(-1)
    batch = tuple(x.shape[:-2])
    xa = x.detach().cpu().to(tA).reshape(-1, N, K).numpy()
    ga = g.detach().cpu().to(tA).reshape(-1, M, K).numpy()
    B = xa.shape[0]
    degi = torch.bincount(row, minlength=M).clamp(min=1)
    dega = degi.to(tA).numpy()
    va = None if value is None else value.detach().cpu().to(tA).numpy()

    def rounded(a, shape):
        return torch.from_numpy(np.ascontiguousarray(a)).to(T).reshape(shape)

    # out: entries of a row in order, divided once at the end for mean
    acc = np.zeros((M, B, K), dtype=A)
    contrib = xa[:, c, :].transpose(1, 0, 2)
    if va is not None:
        contrib = va[:, None, None] * contrib
    np.add.at(acc, r, contrib.astype(A))
    if reduce == 'mean':
        acc = acc / dega[:, None, None]
    out = rounded(acc.transpose(1, 0, 2), (*batch, M, K))
    # grad_value: batches, then features, in order
    prod = (xa[:, c, :] * ga[:, r, :]).transpose(1, 0, 2).reshape(r.size, B * K).astype(A)
    gv = np.cumsum(prod, axis=1, dtype=A)[:, -1] if B * K > 0 else np.zeros(r.size, dtype=A)
    if reduce == 'mean':
        gv = gv / dega[r]
    gv = rounded(gv, (r.size, ))
    # grad_mat: the weight in T first
    if reduce == 'mean':
        cnt = degi[row].to(T)
        wT = cnt.reciprocal() if value is None else value.detach().cpu() / cnt
    else:
        wT = None if value is None else value.detach().cpu()
    acc = np.zeros((N, B, K), dtype=A)
    contrib = ga[:, r, :].transpose(1, 0, 2)
    if wT is not None:
        contrib = wT.to(tA).numpy()[:, None, None] * contrib
    np.add.at(acc, c, contrib.astype(A))
    gm = rounded(acc.transpose(1, 0, 2), (*batch, N, K))
    return out, gv, gm


# ---- graphs -----------------------------------------------------------------------------------------------------
def _graph(deg, cols, N, hub_row=-1, hub_col=-1):
    deg = np.asarray(deg, dtype=np.int64)
    rowptr = np.zeros(deg.size + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.concatenate([np.asarray(c, dtype=np.int64) for c in cols] + [np.zeros(0, dtype=np.int64)])
    assert col.size == rowptr[-1] and (col.size == 0 or (col.min() >= 0 and col.max() < N))
    row = np.repeat(np.arange(deg.size, dtype=np.int64), deg)
    unref = np.setdiff1d(np.arange(N), col)
    return Graph(torch.from_numpy(row), torch.from_numpy(col), torch.from_numpy(rowptr), int(deg.size), N, hub_row,
                 hub_col, torch.from_numpy(unref))


def _runs_of_zero(deg):
    best = run = 0
    for d in deg:
        run = run + 1 if d == 0 else 0
        best = max(best, run)
    return best


def edge_graph():
    """619 x 257, 2125 entries in CSR order (columns ascending inside a row).  The properties the backward tests rely
    on are asserted below.  No (row, col) pair repeats outside the hub row; the hub row has more entries (720) than
    the matrix has columns, so its columns necessarily repeat (three entries per referenced column)."""
    rs = np.random.RandomState(7)
    N, hub_col = 257, 3
    never = np.concatenate([[5, 100], np.arange(232, N)])
    usable = np.setdiff1d(np.arange(N), np.concatenate([never, [hub_col]]))
    small = list(range(12)) + list(range(11, -1, -1)) + [1 + (i % 3) for i in range(541)]
    deg = [0, 0, 0, 720, 63, 64, 65] + [0] * 41 + small + [0] * 6
    hub_row = 3
    cols = []
    for m, d in enumerate(deg):
        if m == hub_row:
            c = np.concatenate([np.repeat(usable, 3), np.full(d - 3 * usable.size, hub_col)])
        elif d == 0:
            c = np.zeros(0, dtype=np.int64)
        else:
            c = np.concatenate([[hub_col], rs.choice(usable, d - 1, replace=False)])
        cols.append(np.sort(c))
    G = _graph(deg, cols, N, hub_row, hub_col)
    deg = np.asarray(deg)
    E = G.col.numel()
    assert 200 <= G.M <= 999 and G.N == 257 and 2000 <= E <= 3000
    assert (deg[:3] == 0).all() and deg[3] > 0, 'three leading empty rows'
    assert deg[hub_row] >= 700 and deg[hub_row] > 10 * 64, 'hub row'
    assert all((deg == d).sum() >= 1 for d in (63, 64, 65)), 'rows of 63 / 64 / 65 entries'
    assert _runs_of_zero(deg[3:-6]) >= 40, 'a run of empty rows inside the matrix'
    assert all((deg == d).sum() >= 1 for d in range(12)), 'rows of 0 ... 11 entries'
    assert (deg[-5:] == 0).all(), 'trailing empty rows'
    colcount = torch.bincount(G.col, minlength=N)
    assert int(colcount[hub_col]) > 512 and int(colcount.argmax()) == hub_col, 'hub column'
    assert G.unreferenced.numel() >= 20 and bool((colcount[G.unreferenced] == 0).all()), 'unreferenced columns'
    assert E % 64 != 0 and E % 256 != 0, 'a tail wave and a tail block'
    key = (G.row * N + G.col).numpy()
    outside = key[G.row.numpy() != hub_row]
    assert np.unique(outside).size == outside.size, 'a repeated (row, col) pair outside the hub row'
    assert bool((G.rowptr[1:] - G.rowptr[:-1] == torch.from_numpy(deg)).all())
    return G


def tiny_graphs():
    """One graph per E in {1, 63, 64, 65, 255, 256, 257}: six rows, the first and the last empty, no repeated pair."""
    out = []
    N = 131
    for E in (1, 63, 64, 65, 255, 256, 257):
        a = E - E // 2
        b = E // 2 - E // 8
        c = E - a - b
        deg = [0, a, 0, b, c, 0]
        rs = np.random.RandomState(E)
        cols = [np.sort(rs.choice(N, d, replace=False)) for d in deg]
        G = _graph(deg, cols, N)
        assert G.col.numel() == E and deg[0] == 0 and deg[-1] == 0 and G.M == 6
        key = (G.row * N + G.col).numpy()
        assert np.unique(key).size == E
        out.append(G)
    assert [g.col.numel() for g in out] == [1, 63, 64, 65, 255, 256, 257]
    return out


def cache_graph():
    """4096 x 4096 with 256 entries in every row (2^20 in all, columns drawn with a cubic skew towards the low ids,
    repeats allowed): the smallest problem on which the forward keeps a relabelled copy of its dense operand
    (relabel_possible, csrc/spmm_kernels.h: E >= 2^20, N >= 4096, E >= 8 N; rows of a power-of-two size >= 256 bytes
    are the caller's part)."""
    rs = np.random.RandomState(11)
    M = N = 4096
    col = np.sort(np.minimum((rs.rand(M, 256) ** 3 * N).astype(np.int64), N - 1), axis=1)
    G = _graph(np.full(M, 256), list(col), N, -1, 0)
    E = G.col.numel()
    assert E >= 1 << 20 and N >= 4096 and E >= 8 * N
    assert int(torch.bincount(G.col, minlength=N).argmax()) == 0 and int((G.col == 0).sum()) > 10000, 'hub column'
    return G


def cache_width(dtype):
    """The narrowest K whose rows are a power of two of at least 256 bytes."""
    return 256 // element_size(dtype)


def random_graph(M, N, E, seed):
    """E distinct (row, col) pairs drawn uniformly, in CSR order."""
    rs = np.random.RandomState(seed)
    key = np.sort(rs.choice(M * N, E, replace=False))
    deg = np.bincount(key // N, minlength=M)
    cols = [key[key // N == m] % N for m in range(M)]
    return _graph(deg, cols, N)


def csc_arrays(G):
    """(colptr, csr2csc) by a stable host argsort of the column ids: independent of the product's own sort."""
    perm = torch.from_numpy(np.argsort(G.col.numpy(), kind='stable'))
    colptr = torch.zeros(G.N + 1, dtype=torch.int64)
    colptr[1:] = torch.cumsum(torch.bincount(G.col, minlength=G.N), 0)
    return colptr, perm


# ---- widths -----------------------------------------------------------------------------------------------------
def element_size(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def vector_widths(dtype):
    """K = slots * (16 / es): rows made of whole 16-byte packets."""
    return [s * (16 // element_size(dtype)) for s in VECTOR_SLOTS]


def scalar_widths(dtype):
    """The K whose rows are no whole number of 16-byte packets."""
    return [K for K in SCALAR_K if (K * element_size(dtype)) % 16 != 0]


def value_bw_launch(K, dtype, aligned=True):
    """launch_value_bw's rule restated (csrc/spmm_bw.hip) -> (lanes per row, trips of the slot loop)."""
    es = element_size(dtype)
    vec = 16 // es if (K > 0 and (K * es) % 16 == 0 and aligned) else 1
    slots = -(-K // vec)
    lpr = 1
    while lpr < min(slots, 64):
        lpr *= 2
    return lpr, -(-slots // lpr)


# ---- inputs -----------------------------------------------------------------------------------------------------
def edge_values(E, dtype, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(E, generator=g) - 0.3).to(dtype)


def integer_inputs(G, K, dtype, seed, batch=(), with_value=False):
    """x, g with integer elements in [-3, 3] (and values in {1, 2}): every product and every partial sum is an
    integer below 2^24, exact in an fp32 / fp64 accumulator in any order, and every exact result stays inside the
    fp16 range -- a correct kernel returns exact.to(dtype) bit for bit."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (*batch, G.N, K), generator=gen).to(dtype)
    g = torch.randint(-3, 4, (*batch, G.M, K), generator=gen).to(dtype)
    v = torch.randint(1, 3, (G.col.numel(), ), generator=gen).to(dtype) if with_value else None
    B = 1
    for b in batch:
        B *= b
    rowcount = int(torch.bincount(G.row, minlength=G.M).max()) if G.row.numel() else 0
    colcount = int(torch.bincount(G.col, minlength=G.N).max()) if G.col.numel() else 0
    worst = max(9 * K * B, 3 * 2 * rowcount, 3 * 2 * colcount)
    assert worst < FP16_MAX and worst < 2 ** 24
    return x, g, v
