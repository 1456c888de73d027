"""SparseTensor.gatv2_attention (csrc/gatv2.hip) against plain float64 torch on the CPU: out and lse through the public call
and through the C entry point (guarded buffers over a sentinel-filled workspace) inside the derived bound of
tests/fused_attention_reference.py with the GATv2 score term, the three gradients against float64 autograd with the
float32 unfused chain as the yardstick, shared weights, and equal bits of two calls.  One pattern per case, sized from
the route's chunk L: empty first, inner and last rows, a row of exactly L entries that ends on a chunk edge, a hub row of
2 L + 3 entries (tail record, a whole chunk, head record) whose largest score sits in its last chunk, repeated columns,
and one element with x_src == -x_dst exactly."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import fused_attention_reference as F
from tests.util import bits_equal, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
SLOPE = 0.2
U32 = 2.0 ** -24
GUARD = 64
CASES = [(1, 1), (1, 64), (3, 5), (8, 8), (2, 40), (70, 4), (1, 'widest')]


def route(dtype, H, D, E=0, offs=(0, 0, 0)):
    w = (ctypes.c_int64 * 7)()
    ptrs = [ctypes.c_void_p(4096 + o) for o in offs]
    assert nat.lib().tsamd_gatv2_route(F.CODE[dtype], H, D, E, *ptrs, w) == 0
    return [int(v) for v in w]


def pattern(L, M=40, N=30):
    """-> (row, col, ptr, hub, e_zero): row 1 holds the entries [0, L), the hub row 3 holds [L + 3, 3 L + 6)."""
    deg = [1 + (r * 7) % 5 for r in range(M)]
    deg[0] = deg[M // 2] = deg[M - 1] = 0
    deg[1], deg[2], deg[3] = L, 3, 2 * L + 3
    row = np.repeat(np.arange(M), deg)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    col = (np.arange(len(row)) * 11 + row) % (N - 1)  # column N - 1 is kept for the hub's last entries
    col[ptr[4] - 4:ptr[4]] = N - 1
    return row, col, ptr, 3, int(ptr[2])


def operands(dtype, H, D, row, col, ptr, hub, e_zero, M=40, N=30, seed=0):
    """float64 tensors whose values the dtype holds exactly."""
    g = torch.Generator().manual_seed(seed + 131 * H + D)
    exact = lambda t: t.to(TORCH[dtype]).double()  # noqa: E731
    xd, xs = exact(torch.randn(M, H, D, generator=g)), exact(torch.randn(N, H, D, generator=g))
    att = exact(torch.randn(H, D, generator=g))
    xs[N - 1] = 4.0 * torch.sign(att) + (att == 0)  # the hub's largest scores: its last chunk
    xd[row[e_zero], 0, 0] = -xs[col[e_zero], 0, 0]  # z == 0 exactly
    s = (torch.nn.functional.leaky_relu(xd[torch.as_tensor(row)] + xs[torch.as_tensor(col)], SLOPE) * att).sum(-1)
    return xd, xs, exact(att * (60.0 / s.abs().amax(0))[:, None])  # the scores of every head reach 60


def reference(row, col, M, xd, xs, att):
    """float64: gathers by row / col, softmax over the row with index_reduce / index_add -> (out, lse, s, z)."""
    row, col = torch.as_tensor(row), torch.as_tensor(col)
    H = xd.size(1)
    z = xd[row] + xs[col]
    s = (torch.nn.functional.leaky_relu(z, SLOPE) * att).sum(-1)
    m = torch.full((M, H), -np.inf, dtype=torch.float64).index_reduce(0, row, s.detach(), 'amax')
    ex = torch.exp(s - m[row])
    l = torch.zeros(M, H, dtype=torch.float64).index_add(0, row, ex)
    out = torch.zeros_like(xd).index_add(0, row, (ex / l[row])[:, :, None] * xs[col])
    return out, (m + torch.log(l)).detach(), s.detach(), z.detach()


def expect_forward(row, col, ptr, xd, xs, att):
    """The comparator's Expect with the score term (D + 3) u sum_d |att| |leaky_relu(z)| in the place of the dot
    product's: mass, and the two sums a1, b1 that carry it."""
    out, lse, s, z = reference(row, col, len(ptr) - 1, xd, xs, att)
    zero = np.zeros(xs.shape)
    ex = F.exact(ptr, col, s.numpy(), np.zeros(xd.shape), zero, xs.numpy(), 1.0)
    assert np.allclose(ex.out, out.detach().numpy(), rtol=1e-12, atol=1e-300)
    mass = (att.abs() * torch.nn.functional.leaky_relu(z, SLOPE).abs()).sum(-1).numpy()
    w = np.abs(xs.numpy()[col]) + np.abs(ex.out[row])
    a1, b1 = np.zeros(ex.a1.shape), np.zeros(ex.b1.shape)
    np.add.at(a1, row, (ex.p * mass)[:, :, None] * w)
    np.add.at(b1, row, ex.p * mass)
    return ex._replace(out=out.detach().numpy(), lse=lse.numpy(), a1=a1, b1=b1, mass=mass), s


def cabi_forward(dev, dtype, ptr, col, xd, xs, att, src_off=0, fill=85):
    """tsamd_gatv2_attention into guarded out and lse over a workspace filled with `fill`; x_src starts src_off elements
    past a 16-byte boundary -> (out, lse)."""
    tdt = TORCH[dtype]
    M, H, D = xd.shape
    N, E = xs.size(0), len(col)
    L = nat.lib()
    dxd, datt = xd.to(dev, tdt).contiguous(), att.to(dev, tdt).contiguous()
    raw_s = torch.zeros(xs.numel() + 16, dtype=tdt, device=dev)
    dxs = raw_s[src_off:src_off + xs.numel()].view(xs.shape).copy_(xs)
    assert dxs.data_ptr() % 16 == src_off * tdt.itemsize
    dptr, dcol = torch.as_tensor(ptr).to(dev), torch.as_tensor(col).to(dev)
    words = route(dtype, H, D, E, (0, src_off * tdt.itemsize, 0))
    nbytes = L.tsamd_gatv2_workspace_bytes(F.CODE[dtype], H, D, E)
    assert nbytes == words[6] and words[0] == (1 if src_off or D % (16 // tdt.itemsize) else 0)
    ws = nat.workspace(nbytes, dev).fill_(fill)
    raw_o = torch.full(((M * H * D + 2 * GUARD) * tdt.itemsize, ), 85, dtype=torch.uint8, device=dev)
    raw_l = torch.full(((M * H + 2 * GUARD) * 4, ), 85, dtype=torch.uint8, device=dev)
    o0, l0 = GUARD * tdt.itemsize, GUARD * 4
    with torch.cuda.device(dev):
        st = L.tsamd_gatv2_attention(F.CODE[dtype], nat._ptr(dptr), nat._ptr(dcol), nat._ptr(dxd), nat._ptr(dxs),
                                     nat._ptr(datt), SLOPE, ctypes.c_void_p(raw_o.data_ptr() + o0), None,
                                     ctypes.c_void_p(raw_l.data_ptr() + l0), M, N, H, D, E, nat._ptr(ws),
                                     ctypes.c_size_t(nbytes), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_gatv2_attention')
    for raw, start in ((raw_o, o0), (raw_l, l0)):
        assert bool((raw[:start] == 85).all()) and bool((raw[-start:] == 85).all()), 'a guard word was written'
    return raw_o[o0:-o0].view(tdt).view(M, H, D).clone(), raw_l[l0:-l0].view(torch.float32).view(M, H).clone()


def chain(A, row, col, xd, xs, att):
    """What a layer writes today, in the library's float32 operators."""
    s = (torch.nn.functional.leaky_relu(xs[col] + xd[row], SLOPE) * att).sum(-1)
    return A.set_value(s, layout='coo').softmax(1).matmul_heads(xs)


def held(got, ref, yard, dtype, what):
    """max |fused - ref| <= 4 max |chain - ref| + 8 u max |ref| (+ 2^-8 |ref| per element for the bfloat16 store)."""
    ref = ref.numpy()
    err = np.abs(got.double().cpu().numpy() - ref)
    bound = 4 * float(np.abs(yard.double().cpu().numpy() - ref).max()) + 8 * U32 * float(np.abs(ref).max())
    bound = bound + (2.0 ** -8 * np.abs(ref) if dtype == 'bf16' else 0.0)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print('%s grad_%s: worst error / bound %.3g' % (dtype, what, ratio))
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('H,D', CASES)
def test_forward_and_gradients_against_float64(dev, dtype, H, D):
    import pytorch_sparse_amd as ts
    tdt = TORCH[dtype]
    D = 64 * (16 // tdt.itemsize) if D == 'widest' else D
    L = route(dtype, H, D)[5]
    row, col, ptr, hub, e_zero = pattern(L)
    xd, xs, att = operands(dtype, H, D, row, col, ptr, hub, e_zero)
    leaves64 = [t.clone().requires_grad_() for t in (xd, xs, att)]
    ex, s = expect_forward(row, col, ptr, xd, xs, att)
    hs = s[ptr[hub]:ptr[hub + 1]]
    assert bool((hs.argmax(0) >= len(hs) - 6).all()) and float(s.abs().max()) > 50.0
    assert float((xd[row[e_zero], 0, 0] + xs[col[e_zero], 0, 0]).abs()) == 0.0

    A = ts.SparseTensor(row=torch.as_tensor(row).to(dev), col=torch.as_tensor(col).to(dev), sparse_sizes=(40, 30),
                        is_sorted=True)
    leaves = [t.to(dev, tdt).requires_grad_() for t in (xd, xs, att)]
    out = A.gatv2_attention(*leaves, SLOPE)
    assert out.shape == (40, H, D) and out.dtype == tdt
    o1, l1 = cabi_forward(dev, dtype, ptr, col, xd, xs, att, fill=85)
    o2, l2 = cabi_forward(dev, dtype, ptr, col, xd, xs, att, fill=0)
    assert bits_equal(o1, o2) and bits_equal(l1, l2) and bits_equal(o1, out.detach()), 'two calls differ'
    ratios = F.check(tonp(o1), tonp(l1), ex, dtype)
    print('%s H %d D %d forward: worst error / bound out %.3g lse %.3g' % (dtype, H, D, *ratios))
    empty = np.diff(ptr) == 0
    assert bool((o1.float().cpu().numpy()[empty] == 0).all()) and bool(np.isneginf(tonp(l1)[empty]).all())

    go = torch.randn(40, H, D, generator=torch.Generator().manual_seed(5)).to(tdt).double()
    want = torch.autograd.grad(reference(row, col, 40, *leaves64)[0], leaves64, go)
    got = torch.autograd.grad(out, leaves, go.to(dev, tdt))
    leaves32 = [t.to(dev, torch.float32).requires_grad_() for t in (xd, xs, att)]
    drow, dcol, _ = A.coo()
    yard = torch.autograd.grad(chain(A, drow, dcol, *leaves32), leaves32, go.to(dev, torch.float32))
    for g, w, y, name in zip(got, want, yard, ('x_dst', 'x_src', 'att')):
        assert g.dtype == tdt and g.shape == w.shape
        held(g, w, y, dtype, name)
    again = torch.autograd.grad(A.gatv2_attention(*leaves, SLOPE), leaves, go.to(dev, tdt))
    assert all(bits_equal(a, b) for a, b in zip(got, again)), 'two backward calls differ'


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_x_src_off_the_boundary_takes_the_generic_route(dev, dtype):
    H, D = 8, 8
    L = route(dtype, H, D)[5]
    row, col, ptr, hub, e_zero = pattern(L)
    xd, xs, att = operands(dtype, H, D, row, col, ptr, hub, e_zero)
    ex, _ = expect_forward(row, col, ptr, xd, xs, att)
    o0, l0 = cabi_forward(dev, dtype, ptr, col, xd, xs, att, src_off=0)
    o1, l1 = cabi_forward(dev, dtype, ptr, col, xd, xs, att, src_off=1)
    F.check(tonp(o0), tonp(l0), ex, dtype)
    F.check(tonp(o1), tonp(l1), ex, dtype)


def test_shared_weights(dev):
    """x_dst is x_src: autograd adds the two gradients."""
    import pytorch_sparse_amd as ts
    H, D = 3, 5
    row, col, ptr, hub, e_zero = pattern(route('f32', H, D)[5], M=30, N=30)
    x, _, att = operands('f32', H, D, row, col, ptr, hub, e_zero, M=30, N=30)
    A = ts.SparseTensor(row=torch.as_tensor(row).to(dev), col=torch.as_tensor(col).to(dev), sparse_sizes=(30, 30),
                        is_sorted=True)
    go = torch.randn(30, H, D, generator=torch.Generator().manual_seed(6)).double()
    x64, a64 = x.clone().requires_grad_(), att.clone().requires_grad_()
    want = torch.autograd.grad(reference(row, col, 30, x64, x64, a64)[0], [x64, a64], go)
    xg, ag = x.to(dev, torch.float32).requires_grad_(), att.to(dev, torch.float32).requires_grad_()
    got = torch.autograd.grad(A.gatv2_attention(xg, xg, ag, SLOPE), [xg, ag], go.to(dev, torch.float32))
    xy, ay = x.to(dev, torch.float32).requires_grad_(), att.to(dev, torch.float32).requires_grad_()
    drow, dcol, _ = A.coo()
    yard = torch.autograd.grad(chain(A, drow, dcol, xy, xy, ay), [xy, ay], go.to(dev, torch.float32))
    for g, w, y, name in zip(got, want, yard, ('x', 'att')):
        held(g, w, y, 'f32', name)
