"""SparseTensor.matmul_multi (csrc/spmm_multi.hip) against a plain fp64 loop.  The bounds are derived in
docs/design/widening.md, "Fused multi-aggregation": with n the entries of a row, L the entries of a chunk
(tsamd_spmm_multi_route) and m = min(n, L),
  sum   (n + 2) u_acc sum|y| + u_T |ref|,   mean the same over n,
  var   (3 m + 12) (m + 1) u_acc var + u_T var   -- no |mean| in it,   std the same relative bound + u_acc;
u_T |ref| is the rounding of the store: half a subnormal step where |ref| is below the normal range (float16)."""
import ctypes
import functools

import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import SparseTensor, _native as nat

pytestmark = pytest.mark.gpu
ALL = ['sum', 'mean', 'min', 'max', 'var', 'std']
M, N, HUB = 300, 200, 2200
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
WIDTHS = [(torch.float32, 1), (torch.float32, 4), (torch.float32, 5), (torch.float32, 256), (torch.float32, 260),
          (torch.bfloat16, 8), (torch.bfloat16, 72), (torch.float16, 16), (torch.float64, 6)]


@functools.lru_cache(None)
def pattern():
    """rows 0-2, 100-109 and 297-299 empty; rows 3-49 hold entries [0, 512), so row 49 ends on a chunk boundary of every
    width; the hub row 50 holds [512, 2712): it starts a chunk, spans several and crosses the tile boundary at 2048; the
    other rows hold 1-3 entries"""
    g = torch.Generator().manual_seed(7)
    deg = torch.randint(1, 4, (M, ), generator=g)
    cuts = torch.cat([torch.zeros(1, dtype=torch.long), (torch.randperm(511, generator=g)[:46] + 1).sort().values,
                      torch.tensor([512])])
    deg[3:50] = cuts[1:] - cuts[:-1]
    deg[50] = HUB
    deg[:3] = 0
    deg[100:110] = 0
    deg[297:] = 0
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    return rowptr, torch.randint(0, N, (int(rowptr[-1]), ), generator=g)


def adj(value=None):
    rowptr, col = pattern()
    return SparseTensor(rowptr=rowptr.cuda(), col=col.cuda(), value=None if value is None else value.cuda(),
                        sparse_sizes=(M, N), is_sorted=True, trust_data=True)


def reference(x, value):
    """fp64, row by row: the six reductions [M, 6, F], first-occurrence winners, sum|y|; differentiable in x"""
    rowptr, col = pattern()
    E = col.numel()
    y = x.double()[col] * (1 if value is None else value.double()[:, None])
    e_id = torch.arange(E)[:, None]
    rows, amin, amax, absum = [], [], [], []
    for m in range(M):
        s, e = int(rowptr[m]), int(rowptr[m + 1])
        p = y[s:e]
        if s == e:
            rows.append(torch.zeros(6, x.size(1), dtype=torch.float64))
            amin.append(torch.full((x.size(1), ), E))
            amax.append(torch.full((x.size(1), ), E))
        else:
            var = p.var(0, unbiased=False)
            rows.append(torch.stack([p.sum(0), p.mean(0), p.min(0).values, p.max(0).values, var,
                                     torch.where(var > 0, var, torch.ones_like(var)).sqrt() * (var > 0)]))
            amin.append(torch.where(p == rows[-1][2], e_id[s:e], E).min(0).values)
            amax.append(torch.where(p == rows[-1][3], e_id[s:e], E).min(0).values)
        absum.append(p.abs().sum(0))
    return torch.stack(rows), torch.stack(amin), torch.stack(amax), torch.stack(absum).detach()


def chunk_entries(dtype, F):
    route = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spmm_multi_route(nat.DTYPES[dtype], 63, F, None, None, 6 * F, F, route) == 0
    return route[4]


def check_forward(out, x, value, dtype, F):
    ref, _, _, absum = reference(x, value)
    out = out.double().cpu()
    rowptr, _ = pattern()
    n = (rowptr[1:] - rowptr[:-1]).double()[:, None]
    ua, ut = (U[dtype] if dtype == torch.float64 else U[torch.float32]), U[dtype]
    m = n.clamp(max=chunk_entries(dtype, F))
    rel = (3 * m + 12) * (m + 1) * ua
    half_sub = torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps / 2  # the store's error on a subnormal

    def stored(r):
        return (ut * r.abs()).clamp(min=half_sub)
    bound = {'sum': (n + 2) * ua * absum + stored(ref[:, 0]),
             'mean': (n + 2) * ua * absum / n.clamp(min=1) + stored(ref[:, 1]),
             'var': rel * ref[:, 4] + stored(ref[:, 4]), 'std': (rel + ua) * ref[:, 5] + stored(ref[:, 5])}
    for i, name in enumerate(ALL):
        if name in ('min', 'max'):
            assert torch.equal(out[:, i], ref[:, i].to(dtype).double()), name
        else:
            err = (out[:, i] - ref[:, i]).abs()
            print(name, 'worst error / bound', float((err / bound[name].clamp(min=1e-300)).max()))
            assert bool((err <= bound[name]).all()), name
    assert bool((out[:, 4] >= 0).all())


@pytest.mark.parametrize('with_value', [False, True])
@pytest.mark.parametrize('dtype,F', WIDTHS)
def test_six_reductions_against_fp64(dtype, F, with_value):
    g = torch.Generator().manual_seed(F)
    x = torch.randn(N, F, generator=g).to(dtype)
    value = torch.randn(pattern()[1].numel(), generator=g).to(dtype) if with_value else None
    out = adj(value).matmul_multi(x.cuda(), ALL)
    assert out.shape == (M, 6, F) and out.dtype == dtype
    check_forward(out, x, value, dtype, F)


def test_operand_off_the_16_byte_boundary():
    x = torch.randn(N, 4, generator=torch.Generator().manual_seed(1))
    xd = torch.empty(N * 4 + 1, device='cuda')[1:].view(N, 4).copy_(x)
    assert xd.data_ptr() % 16 == 4
    check_forward(adj().matmul_multi(xd, ALL), x, None, torch.float32, 4)


@pytest.mark.parametrize('F', [4, 260])
def test_variance_of_offset_data(F):
    # E[y^2] - E[y]^2 would be off by about u * mean^2 = 0.06 against a variance near 1
    x = 1000 + torch.randn(N, F, generator=torch.Generator().manual_seed(2))
    check_forward(adj().matmul_multi(x.cuda(), ALL), x, None, torch.float32, F)


@pytest.mark.parametrize('dtype,F', [(torch.float32, 5), (torch.float32, 260), (torch.bfloat16, 8)])
def test_exact_sums_and_first_winners(dtype, F):
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (4, F), generator=g)[torch.randint(0, 4, (N, ), generator=g)].to(dtype)  # many equal rows
    value = torch.randint(1, 3, (pattern()[1].numel(), ), generator=g).to(dtype)
    ref, amin, amax, _ = reference(x, value)
    a = adj(value)
    rowptr, col, v = a.csr()
    out, argmin, argmax = torch.ops.tsamd.spmm_multi(rowptr, col, v, None, None, None, x.cuda(), 63)
    for i in (0, 2, 3):
        assert torch.equal(out[:, i].cpu(), ref[:, i].to(dtype)), ALL[i]
    assert torch.equal(argmin.cpu(), amin) and torch.equal(argmax.cpu(), amax)
    assert torch.equal(argmin, torch.ops.torch_sparse.spmm_min(rowptr, col, v, x.cuda())[1])
    assert torch.equal(argmax, torch.ops.torch_sparse.spmm_max(rowptr, col, v, x.cuda())[1])
    empty = (pattern()[0][1:] == pattern()[0][:-1]).cuda()
    assert bool((out[empty] == 0).all()) and bool((argmin[empty] == col.numel()).all())
    assert bool((argmax[empty] == col.numel()).all())


@pytest.mark.parametrize('dtype,F', [(torch.float32, 4), (torch.float32, 260), (torch.bfloat16, 72)])
def test_subsets_give_the_bits_of_the_full_call(dtype, F):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, F, generator=g).to(dtype).cuda()
    a = adj(torch.randn(pattern()[1].numel(), generator=g).to(dtype))
    full = a.matmul_multi(x, ALL)
    assert torch.equal(full, ts.matmul_multi(a, x, ALL))
    for subset in (['max'], ['std', 'sum'], ['mean', 'min'], ['add', 'var']):
        want = full[:, [ALL.index('sum' if r == 'add' else r) for r in subset]]
        assert torch.equal(a.matmul_multi(x, subset).view(torch.uint8), want.contiguous().view(torch.uint8)), subset


def test_gradcheck():
    g = torch.Generator().manual_seed(5)
    dense = (torch.rand(7, 6, generator=g) < 0.5).double() * (0.5 + torch.rand(7, 6, generator=g))
    dense[2] = 0
    a = SparseTensor.from_dense(dense.cuda())
    x = torch.randn(6, 3, generator=g, dtype=torch.float64).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: a.matmul_multi(t, ALL), (x, ))
    assert torch.autograd.gradcheck(lambda t: a.matmul_multi(t, ['std', 'max']), (x, ))


@pytest.mark.parametrize('F', [4, 260])
def test_gradient_against_fp64_autograd(F):
    """each term |v_e| * B_e of grad_x[col[e]] carries the relative error of its row's coefficients (the forward's mean
    and std: rel + n u) and of the column's sums (colcount + 4) u; B_e is the coefficient with absolute values"""
    g = torch.Generator().manual_seed(6)
    rowptr, col = pattern()
    x = torch.randn(N, F, generator=g)
    value = torch.randn(col.numel(), generator=g)
    G = torch.randn(M, 6, F, generator=g)
    xd = x.cuda().requires_grad_()
    adj(value).matmul_multi(xd, ALL).backward(G.cuda())
    xr = x.double().requires_grad_()
    ref, amin, amax, _ = reference(xr, value)
    (ref * G.double()).sum().backward()
    ref, Gd, u = ref.detach(), G.double().abs(), U[torch.float32]
    n = (rowptr[1:] - rowptr[:-1]).double().clamp(min=1)[:, None]
    row = torch.repeat_interleave(torch.arange(M), rowptr[1:] - rowptr[:-1])
    m = n.clamp(max=chunk_entries(torch.float32, F))
    rel = ((3 * m + 12) * (m + 1) + n + 8) * u + (torch.bincount(col, minlength=N).max() + 4) * u
    y = (x.double()[col] * value.double()[:, None]).abs()
    spread = (2 * Gd[:, 4] / n + Gd[:, 5] / (n * ref[:, 5].clamp(min=1e-300)))[row] * (y + ref[:, 1].abs()[row])
    e_id = torch.arange(col.numel())[:, None]
    B = (Gd[:, 0][row] + (Gd[:, 1] / n)[row] + spread + Gd[:, 2][row] * (amin[row] == e_id) +
         Gd[:, 3][row] * (amax[row] == e_id))
    bound = torch.zeros(N, F, dtype=torch.float64).index_add_(0, col, rel[row] * value.double().abs()[:, None] * B)
    err = (xd.grad.double().cpu() - xr.grad).abs()
    print('worst error / bound', float((err / bound.clamp(min=1e-300)).max()))
    assert bool((err <= bound).all())


def test_refusals():
    a, x = adj(), torch.randn(N, 4).cuda()
    with pytest.raises(ValueError, match='batched'):
        a.matmul_multi(x.view(N, 2, 2), ['sum'])
    with pytest.raises(ValueError, match='gradient'):
        adj(torch.ones(pattern()[1].numel()).requires_grad_()).matmul_multi(x, ['sum'])
    for bad in (['median'], ['sum', 'add'], ['max', 'max'], []):
        with pytest.raises(ValueError):
            a.matmul_multi(x, bad)
