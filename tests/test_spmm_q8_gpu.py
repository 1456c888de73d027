"""SparseTensor.matmul_q8 and quantize_rows (csrc/spmm_q8.hip) against fp64 and against torch's CPU fp8 conversions.
The bound of the parity test is derived in docs/design/widening.md, "Quantised features": with n the entries of a row,
  |out - ref| <= (n + 3) 2^-24 sum_e |value[e] scale[col[e]] x[col[e], f]|  (+ 2^-8 |out| for a bfloat16 out),
both sides over n for the mean.  The reference uses the DECODED codes: the quantisation error is not in it."""
import ctypes
import functools

import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import SparseTensor, _native as nat

pytestmark = pytest.mark.gpu
N = 200
FP8 = torch.float8_e4m3fn
WIDTHS = [1, 3, 4, 8, 16, 17, 48, 64, 128, 130, 272, 1024]


def route(F, E=0, xq=None, out=None):
    words = (ctypes.c_int64 * 16)()
    assert nat.lib().tsamd_spmm_q8_route(0, F, E, xq, out, words) == 0
    return list(words)


TILE = route(128)[4]


@functools.lru_cache(None)
def layout(name):
    """rowptr of: 'cut' ~4200 entries over 300 rows of 1 .. 27, one of them across the tile boundary (asserted against
    the route where it is used); 'hub' a row longer than two tiles among rows of 1 .. 3; 'empty' empty rows at the start,
    at the end and in runs; 'none' five rows without an entry"""
    g = torch.Generator().manual_seed(11)
    if name == 'cut':
        deg = torch.randint(1, 28, (300, ), generator=g)
        deg[0] += int((deg.cumsum(0) == TILE).any())  # no row may end on the tile boundary: one lies across it
    elif name == 'hub':
        deg = torch.randint(1, 4, (41, ), generator=g)
        deg[20] = 2 * TILE + 100
    elif name == 'empty':
        deg = torch.randint(1, 20, (40, ), generator=g)
        deg[:3] = 0
        deg[10:17] = 0
        deg[25] = 0
        deg[37:] = 0
    else:
        deg = torch.zeros(5, dtype=torch.long)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    return rowptr, torch.randint(0, N, (int(rowptr[-1]), ), generator=g)


@functools.lru_cache(None)
def operands(F):
    """codes without NaN [N, F] (as bytes), scales, and one value per entry of the longest layout"""
    g = torch.Generator().manual_seed(F)
    xq = (torch.randn(N, F, generator=g) * 8).to(FP8).view(torch.uint8)
    return xq, torch.rand(N, generator=g) + 0.5, torch.randn(8200, generator=g)


def adj(name, value=None):
    rowptr, col = layout(name)
    return SparseTensor(rowptr=rowptr.cuda(), col=col.cuda(), value=None if value is None else value.cuda(),
                        sparse_sizes=(rowptr.numel() - 1, N), is_sorted=True, trust_data=True)


def check(name, F, reduce, with_value, with_scale, out_dtype):
    rowptr, col = layout(name)
    M, E = rowptr.numel() - 1, col.numel()
    xq, scale, value = operands(F)
    value = value[:E] if with_value else None
    scale = scale if with_scale else None
    out = adj(name, value).matmul_q8(xq.cuda().view(FP8), None if scale is None else scale.cuda(), reduce, out_dtype)
    assert out.shape == (M, F) and out.dtype == out_dtype
    out = out.double().cpu()
    w = (torch.ones(E) if value is None else value).double() * (torch.ones(N) if scale is None else scale).double()[col]
    y = w[:, None] * xq.view(FP8).float().double()[col]
    n = (rowptr[1:] - rowptr[:-1])
    row = torch.repeat_interleave(torch.arange(M), n)
    ref = torch.zeros(M, F, dtype=torch.float64).index_add_(0, row, y)
    absum = torch.zeros(M, F, dtype=torch.float64).index_add_(0, row, y.abs())
    n = n.double()[:, None]
    if reduce == 'mean':
        ref, absum = ref / n.clamp(min=1), absum / n.clamp(min=1)
    bound = (n + 3) * 2.0 ** -24 * absum + (2.0 ** -8 * out.abs() if out_dtype == torch.bfloat16 else 0)
    err = (out - ref).abs()
    print(name, F, reduce, 'worst error / bound', float((err / bound.clamp(min=1e-300)).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('F', WIDTHS)
def test_every_width_on_cut_rows(F):
    rowptr, L = layout('cut')[0], route(F)[3]
    assert TILE % L == 0 and bool(((rowptr[:-1] < TILE) & (rowptr[1:] > TILE)).any())  # a row across a tile and a chunk
    check('cut', F, 'sum', True, True, torch.float32)


@pytest.mark.parametrize('with_value,with_scale,out_dtype', [(False, False, torch.float32), (True, False, torch.bfloat16),
                                                             (False, True, torch.bfloat16), (True, True, torch.float32)])
@pytest.mark.parametrize('reduce', ['sum', 'mean'])
@pytest.mark.parametrize('name', ['cut', 'hub', 'empty'])
@pytest.mark.parametrize('F', [17, 128])
def test_parity_against_fp64(F, name, reduce, with_value, with_scale, out_dtype):
    check(name, F, reduce, with_value, with_scale, out_dtype)


@pytest.mark.parametrize('out_dtype', [torch.float32, torch.bfloat16])
def test_no_entries_and_no_rows(out_dtype):
    xq = operands(17)[0].cuda().view(FP8)
    out = adj('none').matmul_q8(xq, None, 'mean', out_dtype)
    assert out.shape == (5, 17) and out.dtype == out_dtype and not bool(out.any())
    empty = SparseTensor(rowptr=torch.zeros(1, dtype=torch.long).cuda(), col=torch.zeros(0, dtype=torch.long).cuda(),
                         sparse_sizes=(0, N), is_sorted=True, trust_data=True)
    assert empty.matmul_q8(xq, None, 'sum', out_dtype).shape == (0, 17)


def test_decode_table():
    """all 256 codes through a one-entry row: nothing is rounded, subnormals, both zeros and the two NaN codes included"""
    xq = torch.arange(256, dtype=torch.uint8).view(16, 16).view(FP8)
    eye = SparseTensor(rowptr=torch.arange(17).cuda(), col=torch.arange(16).cuda(), sparse_sizes=(16, 16), is_sorted=True,
                       trust_data=True)
    out, want = eye.matmul_q8(xq.cuda()).cpu(), xq.float()
    torch.testing.assert_close(out, want, rtol=0, atol=0, equal_nan=True)
    differ = (torch.signbit(out) != torch.signbit(want)) & ~want.isnan()  # the sign of a zero too: sums start at -0.0
    assert not bool(differ.any()), differ.nonzero().tolist()


@pytest.mark.parametrize('F', [16, 48])
@pytest.mark.parametrize('offset', [1, 2, 4, 8])
def test_xq_off_the_16_byte_boundary(offset, F):
    """a view at a storage offset takes a narrower packet: the same bits, and the NaN codes behind the last row are
    never read into a sum"""
    xq, scale, value = operands(F)
    buf = torch.full((offset + N * F + 16, ), 0x7f, dtype=torch.uint8, device='cuda')
    buf[offset:offset + N * F] = xq.cuda().flatten()
    view = buf[offset:offset + N * F].view(N, F).view(FP8)
    assert view.data_ptr() % 16 == offset and route(F, 0, view.data_ptr())[0] == {1: 1, 2: 1, 4: 4, 8: 8}[offset]
    a = adj('cut', value[:layout('cut')[1].numel()])
    got, want = a.matmul_q8(view, scale.cuda()), a.matmul_q8(xq.cuda().view(FP8), scale.cuda())
    assert torch.equal(got, want) and not bool(got.isnan().any())


def special_rows(F, dtype):
    """rows 0-7 have absmax 448 (scale 1; negative on odd rows) beside values on exact ties between adjacent codes and on
    subnormal codes; row 8 is zeros; the absmax of row 9 is negative; the rest are ordinary"""
    g = torch.Generator().manual_seed(F)
    pool = torch.tensor([17., 19., -21., 2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10, 2.0 ** -9, 3 * 2.0 ** -9, -7 * 2.0 ** -9,
                         0.0, 2.0 ** -7 + 2.0 ** -10, 416., 432., 0.40625, -0.0])
    x = torch.randn(24, F, generator=g) * torch.logspace(-3, 3, 24)[:, None]
    x[:8] = pool[(torch.arange(8 * F) * 7 % pool.numel())].view(8, F)
    x[:8, 0] = torch.tensor([448., -448.] * 4)
    x[8] = 0
    x[9] = -x[9].abs()
    x[9, F // 2] = -1000.
    return x.to(dtype)


@pytest.mark.parametrize('F', [1, 5, 16, 130])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_quantize_rows_bit_for_bit(dtype, F):
    x = special_rows(F, dtype)
    xf = x.float()
    amax = xf.abs().amax(1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448)
    codes = (xf / scale[:, None]).clamp(-448, 448).to(FP8)
    xq, s = ts.quantize_rows(x.cuda())
    assert xq.dtype == FP8 and xq.shape == x.shape and s.dtype == torch.float32
    assert torch.equal(s.cpu(), scale) and torch.equal(xq.cpu().view(torch.uint8), codes.view(torch.uint8))
    eye = SparseTensor(rowptr=torch.arange(25).cuda(), col=torch.arange(24).cuda(), sparse_sizes=(24, 24), is_sorted=True,
                       trust_data=True)
    assert torch.equal(eye.matmul_q8(xq, s).cpu(), scale[:, None] * codes.float())  # the round trip rounds once


def test_two_calls_give_the_same_bits():
    xq, scale, value = operands(128)
    a = adj('hub', value[:layout('hub')[1].numel()])
    args = (xq.cuda().view(FP8), scale.cuda(), 'mean', torch.bfloat16)
    assert torch.equal(a.matmul_q8(*args), a.matmul_q8(*args))
