"""SparseTensor.matmul_rel (csrc/rel_gemm.hip, csrc/ops_rel.cpp) against plain fp64 torch on the rounded inputs: a loop
over the relations of A_r @ (x @ W_r) with dense A_r, and its fp64 autograd.  The bound of every element is c * u * S,
S the fp64 sum of the absolute values of its terms, u the unit round-off of the dtype, c derived in
docs/design/widening.md, "Relational SpMM" (u32 = 2^-24, narrow = 1 for bfloat16, else 0):
  forward      c = (n + 2 F + Q + 2) u32 / u + 2 narrow     n entries of a pair, Q pairs of a row, at most
  grad_x       c = (d + 2 Fo + 3) u32 / u + narrow          d entries of a column, at most
  grad_weight  c = (n + 2 T + 3) u32 / u + 2 narrow         T pairs of a relation, at most
Tile, chunk and matrix-instruction sizes come from tsamd_rel_gemm_route."""
import ctypes
import functools

import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import SparseTensor, _native as nat

pytestmark = pytest.mark.gpu
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}
DTYPES = [torch.float32, torch.bfloat16]


def route(dtype, P=1000, R=6, F=64, Fo=64):
    out = (ctypes.c_int64 * 16)()
    assert nat.lib().tsamd_rel_gemm_route(nat.DTYPES[dtype], P, R, F, Fo, out) == 0
    return list(out)


TM, CK = route(torch.float32)[0], route(torch.float32)[7]


@functools.lru_cache(None)
def graph(name):
    """-> (M, N, rowptr, col, rel, P): `counts[r]` pairs of relation r on distinct rows, 1-3 entries per pair (`hub`:
    the first pair of relation 0 holds that many), entries of a row shuffled so that rel is unsorted within it; rows
    from `M - 9` on stay empty"""
    counts, M, hub = {
        'tiles0': ([0, 1, TM - 1, TM, TM + 1, 2 * TM + 3], 3 * TM, 0),   # the empty relation first,
        'tiles3': ([1, TM - 1, TM, 0, TM + 1, 2 * TM + 3], 3 * TM, 0),   # in the middle
        'tiles5': ([2 * TM + 3, 1, TM - 1, TM, TM + 1, 0], 3 * TM, 0),   # and last
        'pairs': ([40, 0, 70, 25], 90, 700),                             # a pair longer than a merge-path partition
        'chunks': ([2 * CK + 37, 10, 0, 100], 2 * CK + 60, 0),           # relation 0 spans three chunks of the wgrad
        'single': ([60], 70, 0),
    }[name]
    g = torch.Generator().manual_seed(len(name) + M)
    N = 50
    rows, rels = [], []
    for r, c in enumerate(counts):
        pr = torch.randperm(M - 9, generator=g)[:c]
        mult = torch.randint(1, 4, (c, ), generator=g)
        if hub and r == 0:
            mult[0] = hub
        rows.append(pr.repeat_interleave(mult))
        rels.append(torch.full((int(mult.sum()), ), r))
    row, rel = torch.cat(rows), torch.cat(rels)
    order = torch.argsort(row * row.numel() + torch.randperm(row.numel(), generator=g))
    row, rel = row[order], rel[order]
    rowptr = torch.zeros(M + 1, dtype=torch.long)
    rowptr[1:] = torch.bincount(row, minlength=M).cumsum(0)
    return M, N, rowptr, torch.randint(0, N, (row.numel(), ), generator=g), rel, sum(counts)


def operands(name, dtype, F, Fo, R, valued, integer=False, seed=0):
    M, N, rowptr, col, rel, _ = graph(name)
    g = torch.Generator().manual_seed(seed)
    if integer:
        x, w = torch.randint(-4, 5, (N, F), generator=g), torch.randint(-2, 3, (R, F, Fo), generator=g)
        v = torch.randint(-1, 2, (col.numel(), ), generator=g)
    else:
        x, w, v = torch.randn(N, F, generator=g), torch.randn(R, F, Fo, generator=g), torch.rand(col.numel(), generator=g) + 0.5
    return x.to(dtype), w.to(dtype), (v.to(dtype) if valued else None), torch.randn(M, Fo, generator=g).to(dtype)


def reference(name, x, w, v, reduce, grad=None):
    """fp64 on the CPU -> (out, S) and, with grad, (grad_x, S_x, grad_w, S_w) as well"""
    M, N, rowptr, col, rel, _ = graph(name)
    row = torch.repeat_interleave(torch.arange(M), rowptr[1:] - rowptr[:-1])
    val = torch.ones(col.numel(), dtype=torch.float64) if v is None else v.double()
    if reduce == 'mean':
        val = val / torch.bincount(row * w.size(0) + rel, minlength=M * w.size(0))[row * w.size(0) + rel]
    A = torch.zeros(w.size(0), M, N, dtype=torch.float64).index_put_((rel, row, col), val, accumulate=True)
    Aa = torch.zeros_like(A).index_put_((rel, row, col), val.abs(), accumulate=True)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    out = torch.bmm(A, torch.matmul(xd, wd)).sum(0)
    S = torch.bmm(Aa, torch.matmul(xd.abs(), wd.abs())).sum(0).detach()
    if grad is None:
        return out.detach(), S
    gx, gw = torch.autograd.grad(out, [xd, wd], grad.double())
    ga = grad.double().abs()
    Sx = torch.bmm(Aa.transpose(1, 2), torch.matmul(ga, wd.abs().transpose(1, 2))).sum(0).detach()
    Sw = torch.bmm(torch.matmul(Aa, xd.abs()).transpose(1, 2), ga.expand(w.size(0), -1, -1)).detach()
    return out.detach(), S, gx, Sx, gw, Sw


def constants(name, dtype, F, Fo, R):
    M, N, rowptr, col, rel, _ = graph(name)
    row = torch.repeat_interleave(torch.arange(M), rowptr[1:] - rowptr[:-1])
    pair, n = torch.unique(row * R + rel, return_counts=True)
    Q = int(torch.bincount(pair // R).max())
    T = int(torch.bincount(pair % R).max())
    d = int(torch.bincount(col).max())
    k, narrow = 2.0 ** -24 / U[dtype], int(dtype == torch.bfloat16)
    n = int(n.max())
    return (n + 2 * F + Q + 2) * k + 2 * narrow, (d + 2 * Fo + 3) * k + narrow, (n + 2 * T + 3) * k + 2 * narrow


def inside(got, want, S, c, dtype):
    err = (got.double().cpu() - want).abs()
    bound = c * U[dtype] * S
    print('max error / bound: %.3f' % float((err / bound.clamp_min(1e-300)).max()))
    return bool((err <= bound).all())


def adj(name, v):
    M, N, rowptr, col, rel, _ = graph(name)
    return SparseTensor(rowptr=rowptr.cuda(), col=col.cuda(), value=None if v is None else v.cuda(), sparse_sizes=(M, N),
                        is_sorted=True, trust_data=True), rel.cuda()


def run(name, x, w, v, reduce, grad=None):
    a, rel = adj(name, v)
    xg, wg = x.cuda().requires_grad_(grad is not None), w.cuda().requires_grad_(grad is not None)
    out = a.matmul_rel(xg, wg, rel, reduce)
    if grad is None:
        return out
    out.backward(grad.cuda())
    return out.detach(), xg.grad, wg.grad


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('reduce', ['sum', 'mean'])
@pytest.mark.parametrize('valued', [False, True])
@pytest.mark.parametrize('name', ['tiles0', 'tiles3', 'tiles5', 'pairs'])
def test_forward_and_gradients(name, valued, reduce, dtype):
    """cases 1, 3 and 6: tile edges and shared, unsorted pairs; both gradients through the public call"""
    if name == 'pairs':  # the hub pair is longer than a partition of the SpMM over the pairs
        r = (ctypes.c_int64 * 24)()
        assert nat.lib().tsamd_spmm_route(nat.DTYPES[dtype], 0, 1, graph(name)[5], 50, 24, graph(name)[3].numel(), None,
                                          None, None, 0, None, r) == 0 and r[7] < 700
    F, Fo, R = 24, 40, 4 if name == 'pairs' else 6
    x, w, v, grad = operands(name, dtype, F, Fo, R, valued)
    want = reference(name, x, w, v, reduce, grad)
    out, gx, gw = run(name, x, w, v, reduce, grad)
    c, cx, cw = constants(name, dtype, F, Fo, R)
    assert out.dtype == dtype and gx.dtype == dtype and gw.dtype == dtype
    assert inside(out, want[0], want[1], c, dtype)
    assert inside(gx, want[2], want[3], cx, dtype)
    assert inside(gw, want[4], want[5], cw, dtype)
    empty = [r for r in range(R) if not bool((graph(name)[4] == r).any())]
    assert empty and not bool(gw[empty].any())  # a relation without a pair: exactly zero


WIDTHS = [(1, 1), (8, 8), (24, 40), (64, 128), (136, 136), (1, 136), (136, 1), (64, 8)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['transposed', 'offset'])
@pytest.mark.parametrize('F,Fo', WIDTHS)
def test_widths(F, Fo, layout, dtype):
    """case 2: below one step of the matrix instruction, off its K and N steps, across two Fo-tiles; x and weight as
    .contiguous() copies of transposed views, and as slices 8 bytes off a 16-byte boundary"""
    x, w, v, _ = operands('tiles0', dtype, F, Fo, 6, True, seed=F + Fo)
    want, S = reference('tiles0', x, w, v, 'sum')
    a, rel = adj('tiles0', v)
    if layout == 'transposed':
        xs, ws = x.cuda().t().contiguous().t().contiguous(), w.cuda().transpose(1, 2).contiguous().transpose(1, 2).contiguous()
    else:
        off = 8 // x.element_size()
        xs = torch.cat([x.new_zeros(off), x.flatten()]).cuda()[off:].view_as(x)
        ws = torch.cat([w.new_zeros(off), w.flatten()]).cuda()[off:].view_as(w)
        assert xs.data_ptr() % 16 == 8 and ws.data_ptr() % 16 == 8
    assert inside(a.matmul_rel(xs, ws, rel), want, S, constants('tiles0', dtype, F, Fo, 6)[0], dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact(dtype):
    """integer inputs whose sums stay exactly representable: =="""
    x, w, v, _ = operands('tiles3', dtype, 2, 40, 6, True, integer=True)
    want, S = reference('tiles3', x, w, v, 'sum')
    assert float(S.max()) <= 256
    assert torch.equal(run('tiles3', x, w, v, 'sum').double().cpu(), want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_relation_and_one_per_entry(dtype):
    """case 4: R = 1 is adj.matmul(x) @ weight[0]; R = nnz gives every entry a relation of its own"""
    F, Fo = 24, 40
    x, w, v, _ = operands('single', dtype, F, Fo, 1, True)
    a, rel = adj('single', v)
    want, S = reference('single', x, w, v, 'sum')
    c = constants('single', dtype, F, Fo, 1)[0]
    assert inside(a.matmul_rel(x.cuda(), w.cuda(), rel), want, S, c, dtype)
    assert inside(a.matmul(x.cuda()).float() @ w.cuda()[0].float(), want, S, c + 2, dtype)  # H rounded, then the product
    nnz = rel.numel()
    M, N, rowptr, col, _, _ = graph('single')
    own = torch.randperm(nnz, generator=torch.Generator().manual_seed(1))
    wn = torch.randn(nnz, F, Fo, generator=torch.Generator().manual_seed(2)).to(dtype)
    row = torch.repeat_interleave(torch.arange(M), rowptr[1:] - rowptr[:-1])
    terms = v.double()[:, None] * torch.bmm(x.double()[col][:, None], wn.double()[own])[:, 0]
    S = v.double().abs()[:, None] * torch.bmm(x.double().abs()[col][:, None], wn.double().abs()[own])[:, 0]
    want = torch.zeros(M, Fo, dtype=torch.float64).index_add_(0, row, terms)
    S = torch.zeros(M, Fo, dtype=torch.float64).index_add_(0, row, S)
    assert inside(a.matmul_rel(x.cuda(), wn.cuda(), own.cuda()), want, S, c, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_weight_gradient_chunks(dtype):
    """case 5: relation 0 spans three chunks and its length is no multiple of the K step; relation 2 is empty"""
    F, Fo, R = 24, 40, 4
    assert graph('chunks')[5] > 2 * route(dtype, graph('chunks')[5], R, F, Fo)[7] and (2 * CK + 37) % route(dtype)[6]
    x, w, v, grad = operands('chunks', dtype, F, Fo, R, True)
    want = reference('chunks', x, w, v, 'mean', grad)
    _, gx, gw = run('chunks', x, w, v, 'mean', grad)
    _, cx, cw = constants('chunks', dtype, F, Fo, R)
    assert inside(gw, want[4], want[5], cw, dtype) and inside(gx, want[2], want[3], cx, dtype)
    assert not bool(gw[2].any())


@pytest.mark.parametrize('dtype', DTYPES)
def test_deterministic(dtype):
    x, w, v, grad = operands('tiles0', dtype, 24, 40, 6, True)
    first, second = run('tiles0', x, w, v, 'mean', grad), run('tiles0', x, w, v, 'mean', grad)
    assert all(torch.equal(p, q) for p, q in zip(first, second))


def test_scripted():
    class Free(torch.nn.Module):
        def forward(self, a: SparseTensor, x: torch.Tensor, w: torch.Tensor, rel: torch.Tensor) -> torch.Tensor:
            return ts.matmul_rel(a, x, w, rel, 'mean')

    x, w, v, _ = operands('tiles0', torch.float32, 24, 40, 6, True)
    a, rel = adj('tiles0', v)
    assert torch.equal(torch.jit.script(Free())(a, x.cuda(), w.cuda(), rel), a.matmul_rel(x.cuda(), w.cuda(), rel, 'mean'))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('transposed', [0, 1])
def test_cabi(transposed, dtype):
    """case 7: tsamd_rel_gemm and tsamd_rel_wgrad straight into guarded buffers over a sentinel-filled workspace"""
    L, dt, K, N, G = nat.lib(), nat.DTYPES[dtype], 24, 40, 64
    g = torch.Generator().manual_seed(3)
    counts = torch.tensor([0, TM + 1, 0, 5])
    P, R, n_src, n_dst = int(counts.sum()), 4, 7, int(counts.sum()) + 3
    relptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).cuda()
    sidx = torch.randint(0, n_src, (P, ), generator=g)  # repeats rows
    didx = torch.randperm(n_dst, generator=g)[:P]
    src, go = torch.randn(n_src, K, generator=g).to(dtype), torch.randn(n_dst, N, generator=g).to(dtype)
    w = torch.randn(R, N, K, generator=g).to(dtype) if transposed else torch.randn(R, K, N, generator=g).to(dtype)
    grp = torch.repeat_interleave(torch.arange(R), counts)
    buf = torch.full((G + n_dst * N + G, ), 512.0, device='cuda')
    nbytes = L.tsamd_rel_gemm_workspace_bytes(dt, P, R, K, N)
    ws = torch.full((nbytes, ), 0xA5, dtype=torch.uint8, device='cuda')
    ptrs = [t.cuda() for t in (src, sidx, didx, w)]

    def call(dt_, K_, nbytes_):
        return L.tsamd_rel_gemm(dt_, transposed, ptrs[0].data_ptr(), n_src, ptrs[1].data_ptr(), ptrs[2].data_ptr(),
                                relptr.data_ptr(), ptrs[3].data_ptr(), None, buf.data_ptr() + 4 * G, n_dst, P, R, K_, N,
                                ws.data_ptr(), nbytes_, None)
    assert call(dt, K, nbytes - 1) == 4 and call(dt, 0, nbytes) == 2 and call(dt, 513, nbytes) == 2
    assert call(nat.DTYPES[torch.float16], K, nbytes) == 2
    assert bool((buf == 512.0).all()) and call(dt, K, nbytes) == 0
    torch.cuda.synchronize()
    wd = w.double().transpose(1, 2) if transposed else w.double()
    want = torch.bmm(src.double()[sidx][:, None], wd[grp])[:, 0]
    S = torch.bmm(src.double().abs()[sidx][:, None], wd.abs()[grp])[:, 0]
    got = buf[G:G + n_dst * N].view(n_dst, N).cpu()
    assert inside(got[didx], want, S, 2 * K * 2.0 ** -24 / U[dtype], dtype)
    rest = torch.ones(n_dst, dtype=torch.bool)
    rest[didx] = False
    assert bool((got[rest] == 512.0).all()) and bool((buf[:G] == 512.0).all()) and bool((buf[-G:] == 512.0).all())
    # the weight gradient of the same items: h = src [n_src, K] through sidx, go [n_dst, N] through didx
    gbuf = torch.full((G + R * K * N + G, ), 512.0, device='cuda').to(dtype)
    nbytes = L.tsamd_rel_wgrad_workspace_bytes(dt, P, R, K, N)
    ws = torch.full((nbytes, ), 0xA5, dtype=torch.uint8, device='cuda')
    gptr, god = gbuf.data_ptr() + G * gbuf.element_size(), go.cuda()

    def wgrad(dt_, K_, nbytes_):
        return L.tsamd_rel_wgrad(dt_, ptrs[0].data_ptr(), n_src, ptrs[1].data_ptr(), god.data_ptr(), n_dst,
                                 ptrs[2].data_ptr(), relptr.data_ptr(), gptr, P, R, K_, N, ws.data_ptr(), nbytes_, None)
    assert wgrad(dt, K, nbytes - 1) == 4 and wgrad(dt, 0, nbytes) == 2 and wgrad(dt, 513, nbytes) == 2
    assert wgrad(nat.DTYPES[torch.float64], K, nbytes) == 2 and wgrad(dt, K, nbytes) == 0
    torch.cuda.synchronize()
    terms = torch.bmm(src.double()[sidx][:, :, None], go.double()[didx][:, None])
    want = torch.zeros(R, K, N, dtype=torch.float64).index_add_(0, grp, terms)
    S = torch.zeros(R, K, N, dtype=torch.float64).index_add_(0, grp, terms.abs())
    got = gbuf[G:G + R * K * N].view(R, K, N).cpu()
    assert inside(got, want, S, (2 * P + 1) * 2.0 ** -24 / U[dtype] + (dtype == torch.bfloat16), dtype)
    assert not bool(got[0].any()) and not bool(got[2].any())
    assert bool((gbuf[:G] == 512.0).all()) and bool((gbuf[-G:] == 512.0).all())
