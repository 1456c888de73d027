"""SparseTensor.matmul_rel with a block-diagonal weight [R, B, ci, co] (csrc/rel_blocks.hip) against plain fp64 torch on
the rounded inputs: torch.block_diag of the blocks gives a dense [R, F, Fo] weight for the reference loop of
test_matmul_rel_gpu.py and its fp64 autograd; the weight gradient is read back off the diagonal.  Bounds are those of
docs/design/widening.md, "Bound of the tests", with the contraction length of a block: forward (n + 2 ci + Q + 2),
grad_x (d + 2 co + 3), grad_weight (n + 2 T + 3) -- `constants` with ci and co in the place of F and Fo."""
import ctypes

import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests.test_matmul_rel_gpu import DTYPES, U, adj, constants, graph, inside, reference, run

pytestmark = pytest.mark.gpu
R = 6
SHAPES = [(2, 32, 32), (4, 16, 16), (8, 8, 8), (64, 1, 1), (3, 8, 24), (5, 20, 28), (2, 136, 136), (2, 1, 68), (2, 68, 1),
          (4, 128, 128)]


def route(dtype, P, B, ci, co):
    out = (ctypes.c_int64 * 16)()
    assert nat.lib().tsamd_rel_blocks_route(nat.DTYPES[dtype], P, R, B, ci, co, out) == 0
    return list(out)


def dense(w):
    return torch.stack([torch.block_diag(*blocks) for blocks in w.double()])


def diagonal(d, B):
    ci, co = d.size(1) // B, d.size(2) // B
    return torch.stack([d[:, b * ci:(b + 1) * ci, b * co:(b + 1) * co] for b in range(B)], 1)


def operands(name, dtype, B, ci, co, integer=False):
    M, N, _, col, _, _ = graph(name)
    g = torch.Generator().manual_seed(B * 10000 + ci * 100 + co)
    if integer:
        x, w = torch.randint(-2, 3, (N, B * ci), generator=g), torch.randint(-2, 3, (R, B, ci, co), generator=g)
        v = torch.randint(-1, 2, (col.numel(), ), generator=g)
    else:
        x, w, v = torch.randn(N, B * ci, generator=g), torch.randn(R, B, ci, co, generator=g), torch.rand(col.numel(), generator=g) + 0.5
    return x.to(dtype), w.to(dtype), v.to(dtype), torch.randn(M, B * co, generator=g).to(dtype)


def check(name, dtype, shape, reduce):
    B, ci, co = shape
    x, w, v, grad = operands(name, dtype, B, ci, co)
    want = reference(name, x, dense(w), v, reduce, grad)
    out, gx, gw = run(name, x, w, v, reduce, grad)
    c, cx, cw = constants(name, dtype, ci, co, R)
    assert out.dtype == dtype and gx.dtype == dtype and gw.dtype == dtype and gw.shape == w.shape
    assert inside(out, want[0], want[1], c, dtype)
    assert inside(gx, want[2], want[3], cx, dtype)
    assert inside(gw, diagonal(want[4], B), diagonal(want[5], B), cw, dtype)
    return gw


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('reduce', ['sum', 'mean'])
@pytest.mark.parametrize('shape', SHAPES)
def test_shapes(shape, reduce, dtype):
    """tile edges of the unit table, an empty relation; blocks below, across and above the 32-column instruction block,
    the Fo tile and the K slice"""
    r = route(dtype, graph('tiles0')[5], *shape)
    if shape == (2, 136, 136):
        assert r[9] > r[2] and r[1] * 2 < 2 * 136  # a window longer than one K slice, three Fo tiles
    gw = check('tiles0', dtype, shape, reduce)
    assert not bool(gw[0].any())  # relation 0 of tiles0 has no pair: exactly zero


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(4, 16, 16), (5, 20, 28)])
def test_offset_layout(shape, dtype):
    """x and weight 8 bytes off a 16-byte boundary"""
    B, ci, co = shape
    x, w, v, _ = operands('tiles0', dtype, B, ci, co)
    want, S = reference('tiles0', x, dense(w), v, 'sum')
    a, rel = adj('tiles0', v)
    off = 8 // x.element_size()
    xs = torch.cat([x.new_zeros(off), x.flatten()]).cuda()[off:].view_as(x)
    ws = torch.cat([w.new_zeros(off), w.flatten()]).cuda()[off:].view_as(w)
    assert xs.data_ptr() % 16 == 8 and ws.data_ptr() % 16 == 8
    assert inside(a.matmul_rel(xs, ws, rel), want, S, constants('tiles0', dtype, ci, co, R)[0], dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_block_is_the_dense_call(dtype):
    x, w, v, grad = operands('tiles0', dtype, 1, 24, 40)
    blocks, full = run('tiles0', x, w, v, 'mean', grad), run('tiles0', x, w[:, 0], v, 'mean', grad)
    assert torch.equal(blocks[0], full[0]) and torch.equal(blocks[1], full[1])
    assert blocks[2].shape == w.shape and torch.equal(blocks[2][:, 0], full[2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact(dtype):
    """integer inputs whose sums stay exactly representable: =="""
    x, w, v, _ = operands('tiles3', dtype, 20, 2, 2, integer=True)
    want, S = reference('tiles3', x, dense(w), v, 'sum')
    assert float(S.max()) <= 256
    assert torch.equal(run('tiles3', x, w, v, 'sum').double().cpu(), want)


@pytest.mark.parametrize('dtype', DTYPES)
def test_weight_gradient_chunks(dtype):
    """relation 0 spans three chunks, relation 2 is empty"""
    assert graph('chunks')[5] > 2 * route(dtype, graph('chunks')[5], 3, 8, 24)[7]
    assert not bool(check('chunks', dtype, (3, 8, 24), 'mean')[2].any())


@pytest.mark.parametrize('dtype', DTYPES)
def test_deterministic(dtype):
    x, w, v, grad = operands('tiles0', dtype, 3, 8, 24)
    first, second = run('tiles0', x, w, v, 'mean', grad), run('tiles0', x, w, v, 'mean', grad)
    assert all(torch.equal(p, q) for p, q in zip(first, second))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('transposed', [0, 1])
def test_cabi(transposed, dtype):
    """tsamd_rel_gemm_blocks and tsamd_rel_wgrad_blocks straight into guarded buffers over a sentinel-filled workspace"""
    L, dt, B, ci, co, G = nat.lib(), nat.DTYPES[dtype], 3, 8, 24, 64
    K, N = B * ci, B * co
    g = torch.Generator().manual_seed(3)
    counts = torch.tensor([0, 65, 0, 5])
    P, n_src, n_dst = int(counts.sum()), 7, int(counts.sum()) + 3
    relptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).cuda()
    sidx, didx = torch.randint(0, n_src, (P, ), generator=g), torch.randperm(n_dst, generator=g)[:P]
    src, go = torch.randn(n_src, K, generator=g).to(dtype), torch.randn(n_dst, N, generator=g).to(dtype)
    w = torch.randn(4, B, ci, co, generator=g).to(dtype)
    grp = torch.repeat_interleave(torch.arange(4), counts)
    dev = [t.cuda() for t in (src, sidx, didx, w.transpose(2, 3).contiguous() if transposed else w, go)]
    buf = torch.full((G + n_dst * N + G, ), 512.0, device='cuda')
    nbytes = L.tsamd_rel_gemm_blocks_workspace_bytes(dt, P, 4, B, ci, co)
    ws = torch.full((nbytes, ), 0xA5, dtype=torch.uint8, device='cuda')

    def gemm(dt_, ci_, nbytes_):
        return L.tsamd_rel_gemm_blocks(dt_, transposed, dev[0].data_ptr(), n_src, dev[1].data_ptr(), dev[2].data_ptr(),
                                       relptr.data_ptr(), dev[3].data_ptr(), None, buf.data_ptr() + 4 * G, n_dst, P, 4, B,
                                       ci_, co, ws.data_ptr(), nbytes_, None)
    assert gemm(dt, ci, nbytes - 1) == 4 and gemm(dt, 0, nbytes) == 2 and gemm(dt, 171, nbytes) == 2
    assert gemm(nat.DTYPES[torch.float16], ci, nbytes) == 2
    assert bool((buf == 512.0).all()) and gemm(dt, ci, nbytes) == 0
    torch.cuda.synchronize()
    want = torch.bmm(src.double()[sidx][:, None], dense(w)[grp])[:, 0]
    S = torch.bmm(src.double().abs()[sidx][:, None], dense(w).abs()[grp])[:, 0]
    got = buf[G:G + n_dst * N].view(n_dst, N).cpu()
    assert inside(got[didx], want, S, 2 * ci * 2.0 ** -24 / U[dtype], dtype)
    rest = torch.ones(n_dst, dtype=torch.bool)
    rest[didx] = False
    assert bool((got[rest] == 512.0).all()) and bool((buf[:G] == 512.0).all()) and bool((buf[-G:] == 512.0).all())
    # the weight gradient of the same items: h = src through sidx, go through didx
    gbuf = torch.full((G + w.numel() + G, ), 512.0, device='cuda').to(dtype)
    nbytes = L.tsamd_rel_wgrad_blocks_workspace_bytes(dt, P, 4, B, ci, co)
    ws = torch.full((nbytes, ), 0xA5, dtype=torch.uint8, device='cuda')

    def wgrad(dt_, ci_, nbytes_):
        return L.tsamd_rel_wgrad_blocks(dt_, dev[0].data_ptr(), n_src, dev[1].data_ptr(), dev[4].data_ptr(), n_dst,
                                        dev[2].data_ptr(), relptr.data_ptr(), gbuf.data_ptr() + G * gbuf.element_size(), P,
                                        4, B, ci_, co, ws.data_ptr(), nbytes_, None)
    assert wgrad(dt, ci, nbytes - 1) == 4 and wgrad(dt, 0, nbytes) == 2 and wgrad(dt, 171, nbytes) == 2
    assert wgrad(nat.DTYPES[torch.float16], ci, nbytes) == 2 and wgrad(dt, ci, nbytes) == 0
    torch.cuda.synchronize()
    terms = torch.bmm(src.double()[sidx][:, :, None], go.double()[didx][:, None])
    want = diagonal(torch.zeros(4, K, N, dtype=torch.float64).index_add_(0, grp, terms), B)
    S = diagonal(torch.zeros(4, K, N, dtype=torch.float64).index_add_(0, grp, terms.abs()), B)
    got = gbuf[G:G + w.numel()].view_as(w).cpu()
    assert inside(got, want, S, (2 * P + 1) * 2.0 ** -24 / U[dtype] + (dtype == torch.bfloat16), dtype)
    assert not bool(got[0].any()) and not bool(got[2].any())
    assert bool((gbuf[:G] == 512.0).all()) and bool((gbuf[-G:] == 512.0).all())
