"""csrc/sddmm.hip and csrc/spmm_heads.hip against tests/attention_reference.py: the two C entry points on every shape,
alignment and layout (routes and census asserted on the host first), the operators, SparseTensor.sddmm / matmul_heads
against dense fp64 torch with all four gradients, a whole attention layer, and a scripted module."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import attention_reference as R
from tests.util import bits_equal, fromnp, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
HEADS = (1, 2, 3, 8)
FEATS = (1, 3, 4, 8, 16, 24, 64, 128)
GUARD = 64  # elements before and after the output that no call may touch


@pytest.fixture(scope='module')
def ts(dev):
    import pytorch_sparse_amd
    return pytorch_sparse_amd


def _place(a, tdt, dev, off):
    """A stored numpy array on the device, its first byte at `off` modulo 16."""
    t = fromnp(a, tdt)
    raw = torch.zeros(t.numel() * t.element_size() + 32, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    view = raw[off:off + t.numel() * t.element_size()].view(tdt).view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == off
    return view


def _guarded(numel, tdt, dev, off):
    raw = torch.full(((numel + 2 * GUARD) * tdt.itemsize + 32, ), 85, dtype=torch.uint8, device=dev)
    start = off + GUARD * tdt.itemsize
    return raw, start, ctypes.c_void_p(raw.data_ptr() + start)


def _read(raw, start, shape, tdt):
    n = int(np.prod(shape)) * tdt.itemsize
    assert bool((raw[:start] == 85).all()) and bool((raw[start + n:] == 85).all()), 'a byte outside the output was written'
    return raw[start:start + n].clone().view(tdt).view(shape)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def call_sddmm(dev, dtype, case_arrays, q, k, scale, with_row, off=0, status=0):
    """tsamd_sddmm_heads through ctypes into the middle of a pre-filled buffer -> the [E, H] scores (stored elements)."""
    ptr, ind, perm = case_arrays
    tdt = TORCH[dtype]
    E, H, D = len(ind), q.shape[1], q.shape[2]
    row = R._seg_of(ptr, q.shape[0], E) if with_row else None
    dq, dk = _place(q, tdt, dev, off), _place(k, tdt, dev, off)
    dptr, dind, dperm, drow = (_dev(a, dev) for a in (ptr, ind, perm, row))
    raw, start, out = _guarded(E * H, tdt, dev, 0)
    with torch.cuda.device(dev):
        st = nat.lib().tsamd_sddmm_heads(R.CODE[dtype], nat._ptr(drow), nat._ptr(dptr), nat._ptr(dind), nat._ptr(dperm),
                                         nat._ptr(dq), nat._ptr(dk), float(scale), out, q.shape[0], k.shape[0], H, D, E,
                                         nat.stream_ptr(dev))
    assert st == status, nat.lib().tsamd_status_string(st)
    return tonp(_read(raw, start, (E, H), tdt))


def call_spmm(dev, dtype, case_arrays, value, x, nseg, off=0, fill_ws=None):
    """tsamd_spmm_heads through ctypes -> the [nseg, H, D] result (stored elements)."""
    ptr, ind, perm = case_arrays
    tdt = TORCH[dtype]
    E, H, D = len(ind), x.shape[1], x.shape[2]
    dx = _place(x, tdt, dev, off)
    dv = None if value is None else _place(value, tdt, dev, 0)
    dptr, dind, dperm = (_dev(a, dev) for a in (ptr, ind, perm))
    L = nat.lib()
    ws = nat.workspace(L.tsamd_spmm_heads_workspace_bytes(R.CODE[dtype], nseg, H, D, E), dev)
    if fill_ws is not None:
        ws.fill_(fill_ws)  # whatever an earlier call left there must not matter
    raw, start, out = _guarded(nseg * H * D, tdt, dev, off)
    with torch.cuda.device(dev):
        st = L.tsamd_spmm_heads(R.CODE[dtype], nat._ptr(dptr), nat._ptr(dind), nat._ptr(dperm), nat._ptr(dv),
                                nat._ptr(dx), out, nseg, x.shape[0], H, D, E, nat._ptr(ws),
                                ctypes.c_size_t(ws.numel()), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_spmm_heads')
    return tonp(_read(raw, start, (nseg, H, D), tdt))


def _same(a, b):
    return R.same_bits(np.asarray(a), np.asarray(b))


# ---- C-ABI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.FLOATS)
def test_cabi_sddmm_every_shape_and_alignment(dev, dtype):
    """H x D x alignment on a layout of three wave windows; row given and searched, with and without a perm, both
    routes (asserted from the route query), the same bits from a second call, no byte outside the output written."""
    case = R.edge_case(64 * 2 + 9, nsrc=23)
    rng = np.random.default_rng(31)
    perm = rng.permutation(case.E).astype(np.int64)
    worst, routes, n = 0.0, set(), 0
    for H in HEADS:
        for D in FEATS:
            q, k, _ = R.operands(case, dtype, H, D, seed=32 + n, with_value=False)
            nq, nk = R.numbers(q, dtype), R.numbers(k, dtype)
            for off in (0, 8):
                n += 1
                pm = perm if n % 2 else None
                scale = (1.0, 0.37, -2.0)[n % 3]
                route = R.sddmm_route(dtype, H, D, off == 0)
                assert route.generic == R.expected_sddmm_route(dtype, H, D, off == 0)
                routes.add(route.generic)
                arrays = (case.ptr, case.ind, pm)
                got = call_sddmm(dev, dtype, arrays, q, k, scale, with_row=n % 4 < 2, off=off)
                again = call_sddmm(dev, dtype, arrays, q, k, scale, with_row=n % 4 >= 2, off=off)
                assert _same(got, again), ('row given and row searched differ', H, D, off)
                try:
                    worst = max(worst, R.check(got, R.sddmm_exact(case.ptr, case.ind, pm, nq, nk, scale), dtype))
                except AssertionError as exc:
                    raise AssertionError('%s: %s' % ((H, D, off, pm is not None), exc)) from None
    assert routes == {0, 1}
    print('%s sddmm: worst err / bound %.3g' % (dtype, worst))


@pytest.mark.parametrize('dtype', R.FLOATS)
def test_cabi_spmm_every_shape_and_alignment(dev, dtype):
    """H x D x alignment on the hub layout of that shape's chunk length (census asserted): rows inside a chunk, cut
    once, spanning three chunks and more, empty leading and trailing rows, a tile boundary."""
    rng = np.random.default_rng(33)
    worst, routes, n = 0.0, set(), 0
    for H in HEADS:
        for D in FEATS:
            r = R.spmm_route(dtype, H, D)
            case = R.hub_case(r.chunk, r.tile)
            c = R.census(case, r.chunk, r.tile, r.staged)
            assert c['span3'] >= 1 and c['cut'] >= 1 and c['inside'] >= 3 and c['empty'] >= 6, c
            _, x, v = R.operands(case, dtype, H, D, seed=34 + n)
            nx, nv = R.numbers(x, dtype), R.numbers(v, dtype)
            n += 1
            pm = rng.permutation(case.E).astype(np.int64) if n % 2 else None
            vv, nvv = (None, None) if n % 5 == 0 else (v, nv)
            expect = R.spmm_exact(case.ptr, case.ind, pm, nvv, nx, case.nseg)
            arrays = (case.ptr, case.ind, pm)
            for off in (0, 8):
                route = R.spmm_route(dtype, H, D, off == 0)
                assert route.generic == R.expected_spmm_route(dtype, H, D, off == 0) and route.chunk == r.chunk
                routes.add(route.generic)
                got = call_spmm(dev, dtype, arrays, vv, x, case.nseg, off=off, fill_ws=85)
                assert _same(got, call_spmm(dev, dtype, arrays, vv, x, case.nseg, off=off, fill_ws=0)), (H, D, off)
                assert bool((R.numbers(got, dtype)[np.diff(case.ptr) == 0] == 0).all()), 'rows without entries are zeros'
                try:
                    worst = max(worst, R.check(got, expect, dtype))
                except AssertionError as exc:
                    raise AssertionError('%s: %s' % ((H, D, off, pm is not None), exc)) from None
    assert routes == {0, 1}
    print('%s spmm: worst err / bound %.3g' % (dtype, worst))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_cabi_every_tile_edge_and_layout(dev, dtype):
    """E = 1 and every chunk / window / workgroup / tile size minus one, exact, plus one; the census layouts (hub, more
    segments in a tile than LDS holds, a single source row)."""
    H, D = 3, 8
    sd, sh = R.sddmm_route(dtype, H, D), R.spmm_route(dtype, H, D)
    sizes = R.edge_sizes(sh.chunk, sd.window, sd.block, sh.tile)
    assert 1 in sizes and sh.chunk + 1 in sizes and sh.tile - 1 in sizes and sd.window - 1 in sizes
    cases = [R.edge_case(E) for E in sizes] + R.assert_census(dtype, H, D)
    rng = np.random.default_rng(35)
    worst_s = worst_m = 0.0
    for i, case in enumerate(cases):
        q, k, v = R.operands(case, dtype, H, D, seed=36 + i)
        nq, nk, nv = (R.numbers(a, dtype) for a in (q, k, v))
        pm = rng.permutation(case.E).astype(np.int64) if i % 2 else None
        arrays = (case.ptr, case.ind, pm)
        try:
            got = call_sddmm(dev, dtype, arrays, q, k, 0.5, with_row=i % 3 == 0)
            worst_s = max(worst_s, R.check(got, R.sddmm_exact(case.ptr, case.ind, pm, nq, nk, 0.5), dtype))
            got = call_spmm(dev, dtype, arrays, v, k, case.nseg, fill_ws=85)
            worst_m = max(worst_m, R.check(got, R.spmm_exact(case.ptr, case.ind, pm, nv, nk, case.nseg), dtype))
            assert _same(got, call_spmm(dev, dtype, arrays, v, k, case.nseg, fill_ws=0)), 'not deterministic'
        except AssertionError as exc:
            raise AssertionError('%s: %s' % (case.name, exc)) from None
    print('%s layouts: worst err / bound sddmm %.3g spmm %.3g' % (dtype, worst_s, worst_m))


def test_cabi_degenerate_shapes(dev):
    L = nat.lib()
    fake = ctypes.c_void_p(0x1000)
    stream = nat.stream_ptr(dev)
    for E, M, H, D in ((0, 4, 2, 3), (0, 0, 2, 3), (5, 4, 0, 3), (5, 4, 2, 0)):
        assert L.tsamd_sddmm_heads(0, None, fake, fake, None, fake, fake, 1.0, fake, M, 4, H, D, E, stream) == 0
    ptr = torch.zeros(5, dtype=torch.int64, device=dev)
    out = torch.full((4, 2, 3), 7.0, device=dev)
    with torch.cuda.device(dev):
        assert L.tsamd_spmm_heads(0, nat._ptr(ptr), None, None, None, None, nat._ptr(out), 4, 4, 2, 3, 0, None,
                                  ctypes.c_size_t(0), stream) == 0
    assert bool((out == 0).all()), 'E = 0 zero-fills the output'
    for M, H, D in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        assert L.tsamd_spmm_heads(0, fake, fake, None, None, fake, None, M, 4, H, D, 5, None, ctypes.c_size_t(0),
                                  stream) == 0
    for tdt in (torch.int32, torch.int64):
        assert L.tsamd_sddmm_heads(nat.DTYPES[tdt], None, fake, fake, None, fake, fake, 1.0, fake, 4, 4, 2, 3, 5,
                                   stream) == 2


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_inputs_stay_in_their_head_row_and_column(dev, bad):
    H, D, dtype = 3, 8, 'f32'
    r = R.spmm_route(dtype, H, D)
    case = R.hub_case(r.chunk, r.tile)
    q, k, v = R.operands(case, dtype, H, D, seed=41)
    q, k = np.abs(q) + 0.5, np.abs(k) + 0.5  # no 0 * inf, no inf - inf: the poisoned outputs are known by position
    hub = int(np.argmax(np.diff(case.ptr)))
    row = R._seg_of(case.ptr, case.nseg, case.E)
    # SDDMM: q[hub + 2] (a row of one entry beside the hub), head 1; k[5], head 2
    one = hub + 2
    assert case.ptr[one + 1] - case.ptr[one] == 1
    q2, k2 = q.copy(), k.copy()
    q2[one, 1, 3] = bad
    k2[5, 2, 0] = bad
    stored = call_sddmm(dev, dtype, (case.ptr, case.ind, None), q2, k2, 1.0, with_row=False)
    got = R.numbers(stored, dtype)
    want = np.zeros((case.E, H), bool)
    want[row == one, 1] = True
    want[case.ind == 5, 2] = True
    assert want[:, 2].sum() >= 2 and np.array_equal(~np.isfinite(got), want)
    R.check(stored, R.sddmm_exact(case.ptr, case.ind, None, q2, k2, 1.0), dtype)
    # SpMM: x[5], head 2 reaches the rows that hold an entry gathering row 5 -- not the neighbours that share a chunk
    # or a record with them; a value of the row of one entry reaches that row only
    x2, v2 = k.copy(), np.abs(v) + 0.5
    x2[5, 2, 1] = bad
    e_one = int(case.ptr[one])
    v2[e_one, 0] = bad
    stored = call_spmm(dev, dtype, (case.ptr, case.ind, None), v2, x2, case.nseg)
    got = R.numbers(stored, dtype)
    want = np.zeros((case.nseg, H, D), bool)
    want[np.unique(row[case.ind == 5]), 2, 1] = True
    want[one, 0, :] = True
    assert want[hub, 2, 1], 'the hub gathers row 5: its neighbours of length 0 and 1 share its chunk'
    assert np.array_equal(~np.isfinite(got), want)
    R.check(stored, R.spmm_exact(case.ptr, case.ind, None, v2, x2, case.nseg), dtype)
    assert want.reshape(case.nseg, -1).any(1).sum() < case.nseg - 10, 'most rows stay finite'


# ---- operators and the Python surface ----------------------------------------------------------------------------------
def _pattern():
    """300 x 200, rows 7..11 and columns 50..59 empty, row 123 a hub that holds every other column."""
    rng = np.random.default_rng(12)
    mask = rng.random((300, 200)) < 0.04
    mask[123] = True
    mask[7:12] = False
    mask[:, 50:60] = False
    row, col = np.nonzero(mask)
    return mask, row, col


@pytest.fixture(scope='module')
def pattern():
    return _pattern()


def _adj(ts, dev, pattern, value=None):
    mask, row, col = pattern
    return ts.SparseTensor(row=torch.from_numpy(row).to(dev), col=torch.from_numpy(col).to(dev), value=value,
                           sparse_sizes=mask.shape)


def _dense_scores(row, col, q, k, scale):
    return (torch.einsum('mhd,nhd->mnh', q, k) * scale)[torch.from_numpy(row), torch.from_numpy(col)]


def _dense_matmul(mask, row, col, v, x):
    A = torch.zeros(mask.shape + (v.shape[1], ), dtype=v.dtype)
    return torch.einsum('mnh,nhd->mhd', A.index_put((torch.from_numpy(row), torch.from_numpy(col)), v), x)


@pytest.mark.parametrize('D', [5, 16])
def test_operators_against_the_oracle(ts, dev, pattern, D):
    mask, row, col = pattern
    H = 3
    A = _adj(ts, dev, pattern)
    rowptr, colidx, _ = A.csr()
    case = R.Case('pattern', tonp(rowptr), tonp(colidx), row.size, 300, 200)
    colptr, row_csc, csr2csc = R.csc_of(case)
    q, k, v = R.operands(case, 'f32', H, D, seed=51)
    dq, dk, dv = (torch.from_numpy(a).to(dev) for a in (q, k, v))
    got = torch.ops.tsamd.sddmm_heads(None, rowptr, colidx, None, dq, dk, 0.25)
    assert got.shape == (row.size, H) and not got.requires_grad
    R.check(tonp(got), R.sddmm_exact(case.ptr, case.ind, None, q, k, 0.25), 'f32')
    assert bits_equal(got, torch.ops.tsamd.sddmm_heads(A.storage.row(), rowptr, colidx, None, dq, dk, 0.25))
    through = torch.ops.tsamd.sddmm_heads(None, _dev(colptr, dev), _dev(row_csc, dev), _dev(csr2csc, dev), dk, dq, 0.25)
    R.check(tonp(through), R.sddmm_exact(case.ptr, case.ind, None, q, k, 0.25), 'f32')
    out = torch.ops.tsamd.spmm_heads(rowptr, colidx, None, dv, dk, 300)
    assert out.shape == (300, H, D)
    R.check(tonp(out), R.spmm_exact(case.ptr, case.ind, None, v, k, 300), 'f32')
    out = torch.ops.tsamd.spmm_heads(_dev(colptr, dev), _dev(row_csc, dev), _dev(csr2csc, dev), dv, dq, 200)
    R.check(tonp(out), R.spmm_exact(colptr, row_csc, csr2csc, v, q, 200), 'f32')
    ones = torch.ops.tsamd.spmm_heads(rowptr, colidx, None, None, dk, 300)
    R.check(tonp(ones), R.spmm_exact(case.ptr, case.ind, None, None, k, 300), 'f32')
    # non-contiguous operands are made contiguous
    wide = torch.from_numpy(np.concatenate([q, q], 2)).to(dev)[:, :, :D]
    assert not wide.is_contiguous()
    assert bits_equal(torch.ops.tsamd.sddmm_heads(None, rowptr, colidx, None, wide, dk, 0.25), got)


@pytest.mark.parametrize('tdt', [torch.float64, torch.float32])
@pytest.mark.parametrize('D', [5, 16])
def test_sparse_tensor_calls_against_dense_fp64(ts, dev, pattern, tdt, D):
    mask, row, col = pattern
    H = 3
    rng = np.random.default_rng(52)
    q, k, v = (torch.from_numpy(rng.standard_normal(s)).to(tdt) for s in ((300, H, D), (200, H, D), (row.size, H)))
    A = _adj(ts, dev, pattern, value=torch.full((row.size, ), 9.0, device=dev))  # the values are not read
    S = A.sddmm(q.to(dev), k.to(dev), 0.3)
    assert isinstance(S, ts.SparseTensor) and S.sparse_sizes() == A.sparse_sizes()
    assert S.storage.rowptr() is A.storage.rowptr(), 'caches are shared'
    got = S.storage.value()
    assert got.shape == (row.size, H) and got.dtype == tdt
    name = 'f64' if tdt == torch.float64 else 'f32'
    case = R.Case('pattern', tonp(A.storage.rowptr()), col.astype(np.int64), row.size, 300, 200)
    R.check(tonp(got), R.sddmm_exact(case.ptr, case.ind, None, q.numpy(), k.numpy(), 0.3), name)
    want = _dense_scores(row, col, q.double(), k.double(), 0.3)
    assert torch.allclose(got.double().cpu(), want, rtol=1e-12 if tdt == torch.float64 else 1e-4, atol=1e-5)
    assert bits_equal(ts.sddmm(A, q.to(dev), k.to(dev), 0.3).storage.value(), got)
    flat = A.sddmm(q[:, 0].to(dev), k[:, 0].to(dev))  # [M, D] operands: one score per entry
    assert flat.storage.value().shape == (row.size, )
    assert bits_equal(flat.storage.value(), A.sddmm(q[:, :1].to(dev), k[:, :1].to(dev)).storage.value()[:, 0])

    B = A.set_value(v.to(dev), layout='coo')
    out = B.matmul_heads(k.to(dev))
    assert out.shape == (300, H, D) and out.dtype == tdt
    R.check(tonp(out), R.spmm_exact(case.ptr, case.ind, None, v.numpy(), k.numpy(), 300), name)
    want = _dense_matmul(mask, row, col, v.double(), k.double())
    assert torch.allclose(out.double().cpu(), want, rtol=1e-12 if tdt == torch.float64 else 1e-4, atol=1e-4)
    assert bool((out[7:12] == 0).all()) and bits_equal(ts.matmul_heads(B, k.to(dev)), out)
    with pytest.raises(Exception):
        B.matmul(k[:, 0].to(dev))  # matmul keeps rejecting 2-D values


def test_all_four_gradients_against_fp64_autograd(ts, dev, pattern):
    mask, row, col = pattern
    H = 3
    rng = np.random.default_rng(53)
    for D in (5, 16):
        q, k, v = (torch.from_numpy(rng.standard_normal(s)) for s in ((300, H, D), (200, H, D), (row.size, H)))
        g = torch.from_numpy(rng.standard_normal((row.size, H)))
        go = torch.from_numpy(rng.standard_normal((300, H, D)))
        dq, dk, dv = (t.clone().requires_grad_() for t in (q, k, v))
        wq, wk = torch.autograd.grad(_dense_scores(row, col, dq, dk, 0.7), (dq, dk), g)
        wv, wx = torch.autograd.grad(_dense_matmul(mask, row, col, dv, dk), (dv, dk), go)
        gq, gk, gv = (t.to(dev).requires_grad_() for t in (q, k, v))
        A = _adj(ts, dev, pattern)
        assert A.storage._colptr is None and A.storage._csr2csc is None
        S = A.sddmm(gq, gk, 0.7).storage.value()
        assert S.requires_grad
        oq, ok = torch.autograd.grad(S, (gq, gk), g.to(dev))
        assert torch.allclose(oq.cpu(), wq, rtol=1e-10, atol=1e-13) and torch.allclose(ok.cpu(), wk, rtol=1e-10, atol=1e-13)
        out = A.set_value(gv, layout='coo').matmul_heads(gk)
        ov, ox = torch.autograd.grad(out, (gv, gk), go.to(dev))
        assert torch.allclose(ov.cpu(), wv, rtol=1e-10, atol=1e-13) and torch.allclose(ox.cpu(), wx, rtol=1e-10, atol=1e-13)
        # float32 inside the comparators
        case = R.Case('pattern', tonp(A.storage.rowptr()), col.astype(np.int64), row.size, 300, 200)
        f = [t.float() for t in (q, k, v, g, go)]
        fq, fk, fv = (t.to(dev).requires_grad_() for t in f[:3])
        oq, ok = torch.autograd.grad(A.sddmm(fq, fk, 0.7).storage.value(), (fq, fk), f[3].to(dev))
        eq, ek = R.sddmm_grads_exact(case.ptr, case.ind, f[0].numpy(), f[1].numpy(), 0.7, f[3].numpy())
        ov, ox = torch.autograd.grad(A.set_value(fv, layout='coo').matmul_heads(fk), (fv, fk), f[4].to(dev))
        ev, ex = R.spmm_grads_exact(case.ptr, case.ind, f[2].numpy(), f[1].numpy(), 300, f[4].numpy())
        ratios = [R.check(tonp(a), b, 'f32') for a, b in ((oq, eq), (ok, ek), (ov, ev), (ox, ex))]
        print('D = %d float32 gradients, worst err / bound: q %.3g k %.3g value %.3g x %.3g' % ((D, ) + tuple(ratios)))


def test_gradcheck_on_a_small_pattern(ts, dev):
    rng = np.random.default_rng(54)
    mask = rng.random((12, 9)) < 0.35
    mask[4] = False
    mask[:, 2] = False
    row, col = np.nonzero(mask)
    A = _adj(ts, dev, (mask, row, col))
    q, k, v = (torch.from_numpy(rng.standard_normal(s)).to(dev).requires_grad_()
               for s in ((12, 2, 3), (9, 2, 3), (row.size, 2)))
    assert torch.autograd.gradcheck(lambda a, b: A.sddmm(a, b, 0.8).storage.value(), (q, k), nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda a, b: A.set_value(a, layout='coo').matmul_heads(b), (v, k), nondet_tol=0.0)
    y = A.sddmm(q, k).storage.value()
    gq, = torch.autograd.grad((y * y).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):  # no second order
        gq.sum().backward()


def test_expanded_and_transposed_grad_out(ts, dev, pattern):
    mask, row, col = pattern
    rng = np.random.default_rng(55)
    H, D = 3, 5
    v, x = torch.from_numpy(rng.standard_normal((row.size, H))), torch.from_numpy(rng.standard_normal((200, H, D)))
    w = torch.from_numpy(rng.standard_normal((300, D, H)))
    A = _adj(ts, dev, pattern)
    for loss in (lambda o, dv: o.sum(), lambda o, dv: (o.transpose(1, 2) * w.to(dv)).sum(),
                 lambda o, dv: (o[:, :, ::2] * 3).sum()):
        gv, gx = v.clone().to(dev).requires_grad_(), x.clone().to(dev).requires_grad_()
        loss(A.set_value(gv, layout='coo').matmul_heads(gx), dev).backward()
        dv, dx = v.clone().requires_grad_(), x.clone().requires_grad_()
        loss(_dense_matmul(mask, row, col, dv, dx), 'cpu').backward()
        assert torch.allclose(gv.grad.cpu(), dv.grad, rtol=1e-10, atol=1e-13)
        assert torch.allclose(gx.grad.cpu(), dx.grad, rtol=1e-10, atol=1e-13)
    gq, gk = (torch.from_numpy(rng.standard_normal(s)).to(dev).requires_grad_() for s in ((300, H, D), (200, H, D)))
    A.sddmm(gq, gk).storage.value().sum().backward()  # an expanded gradient of the scores
    dq, dk = gq.detach().cpu().requires_grad_(), gk.detach().cpu().requires_grad_()
    _dense_scores(row, col, dq, dk, 1.0).sum().backward()
    assert torch.allclose(gq.grad.cpu(), dq.grad, rtol=1e-10, atol=1e-13)
    assert torch.allclose(gk.grad.cpu(), dk.grad, rtol=1e-10, atol=1e-13)


def test_only_the_gradients_asked_for_and_the_column_caches(ts, dev, pattern):
    mask, row, col = pattern
    rng = np.random.default_rng(56)
    H, D = 2, 4
    q, k, v = (torch.from_numpy(rng.standard_normal(s)).to(dev) for s in ((300, H, D), (200, H, D), (row.size, H)))

    def run(which):
        A = _adj(ts, dev, pattern)
        t = {n: a.clone().requires_grad_(n == which) for n, a in (('q', q), ('k', k), ('v', v), ('x', k))}
        if which in ('q', 'k'):
            A.sddmm(t['q'], t['k'], 0.5).storage.value().sum().backward()
        else:
            A = A.set_value(t['v'], layout='coo')  # the caches are built in the storage the call is made on
            A.matmul_heads(t['x']).sum().backward()
        assert [n for n in t if t[n].grad is not None] == [which]
        return A.storage._colptr is None and A.storage._csr2csc is None

    assert run('q') and run('v'), 'no column-side gradient: the CSC caches stay None'
    assert not run('k') and not run('x')
    A = _adj(ts, dev, pattern)
    with torch.no_grad():
        A.sddmm(q.clone().requires_grad_(), k.clone().requires_grad_())
    assert A.storage._colptr is None and A.storage._csr2csc is None


def test_attention_layer_end_to_end(ts, dev, pattern):
    mask, row, col = pattern
    rng = np.random.default_rng(57)
    H, D = 3, 8
    q, k, v = (torch.from_numpy(rng.standard_normal(s)) for s in ((300, H, D), (200, H, D), (200, H, D)))
    w = torch.from_numpy(rng.standard_normal((300, H, D)))
    # dense masked multi-head attention, fp64; rows without entries are left out of the softmax and give zeros
    dq, dk, dv = (t.clone().requires_grad_() for t in (q, k, v))
    scores = torch.einsum('mhd,nhd->mnh', dq, dk) * D ** -0.5
    m3 = torch.from_numpy(mask)[:, :, None].expand_as(scores)
    P = torch.softmax(torch.where(m3, scores, torch.full_like(scores, -np.inf)), 1)
    P = torch.where(m3, P, torch.zeros_like(P))
    want = torch.einsum('mnh,nhd->mhd', P, dv)
    assert bool((want[7:12] == 0).all())
    (want * w).sum().backward()

    A = _adj(ts, dev, pattern)
    gq, gk, gv = (t.to(dev).requires_grad_() for t in (q, k, v))
    attn = A.sddmm(gq, gk, D ** -0.5).softmax(1)
    out = attn.matmul_heads(gv)
    (out * w.to(dev)).sum().backward()
    assert torch.allclose(out.detach().cpu(), want.detach(), rtol=1e-10, atol=1e-13)
    for got, ref in ((gq, dq), (gk, dk), (gv, dv)):
        assert torch.allclose(got.grad.cpu(), ref.grad, rtol=1e-9, atol=1e-12)

    # float32: the multi-head call and the head-by-head composition through matmul, both inside the comparator
    with torch.no_grad():
        fa = A.sddmm(q.float().to(dev), k.float().to(dev), D ** -0.5).softmax(1)
        p32, v32 = fa.storage.value(), v.float().to(dev)
        heads = fa.matmul_heads(v32)
        loop = torch.stack([fa.set_value(p32[:, h].contiguous(), layout='coo').matmul(v32[:, h]) for h in range(H)], 1)
    case = R.Case('pattern', tonp(A.storage.rowptr()), col.astype(np.int64), row.size, 300, 200)
    expect = R.spmm_exact(case.ptr, case.ind, None, tonp(p32), tonp(v32), 300)
    a, b = R.check(tonp(heads), expect, 'f32'), R.check(tonp(loop), expect, 'f32')
    print('attention layer float32, worst err / bound: matmul_heads %.3g, loop over heads %.3g' % (a, b))


def test_scripted_module_calls_both_operators(ts, dev, pattern):
    class Layer(torch.nn.Module):
        def forward(self, rowptr: torch.Tensor, col: torch.Tensor, q: torch.Tensor, k: torch.Tensor,
                    v: torch.Tensor, scale: float) -> torch.Tensor:
            s = torch.ops.tsamd.sddmm_heads(None, rowptr, col, None, q, k, scale)
            p = torch.ops.tsamd.segment_softmax(s, None, rowptr, q.size(0))
            return torch.ops.tsamd.spmm_heads(rowptr, col, None, p, v, q.size(0))

    rng = np.random.default_rng(58)
    q, k, v = (torch.from_numpy(rng.standard_normal(s)).float().to(dev) for s in ((300, 2, 8), (200, 2, 8), (200, 2, 8)))
    A = _adj(ts, dev, pattern)
    rowptr, col, _ = A.csr()
    scripted = torch.jit.script(Layer())
    got = scripted(rowptr, col, q, k, v, 0.35)
    assert bits_equal(got, Layer()(rowptr, col, q, k, v, 0.35))
    assert bits_equal(got, A.sddmm(q, k, 0.35).softmax(1).matmul_heads(v))


def test_errors(ts, dev, pattern):
    mask, row, col = pattern
    A = _adj(ts, dev, pattern)
    f = lambda *s: torch.ones(*s, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match='heads'):
        A.sddmm(f(300, 2, 4), f(200, 3, 4))
    with pytest.raises(ValueError, match='heads'):
        A.set_value(f(row.size, 2), layout='coo').matmul_heads(f(200, 3, 4))
    with pytest.raises(ValueError, match='matmul'):
        A.set_value(f(row.size), layout='coo').matmul_heads(f(200, 3, 4))
    with pytest.raises(ValueError, match='matmul'):
        A.matmul_heads(f(200, 3, 4))
    with pytest.raises(ValueError, match='floating'):
        A.sddmm(f(300, 2, 4).long(), f(200, 2, 4).long())
    with pytest.raises(ValueError, match='floating'):
        A.set_value(f(row.size, 2).long(), layout='coo').matmul_heads(f(200, 2, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        A.sddmm(torch.ones(300, 2, 4), torch.ones(200, 2, 4))
    with pytest.raises(RuntimeError, match='GPU'):
        A.set_value(f(row.size, 2), layout='coo').matmul_heads(torch.ones(200, 2, 4))
    with pytest.raises(ValueError, match='rows'):
        A.sddmm(f(299, 2, 4), f(200, 2, 4))
    with pytest.raises(ValueError, match='columns'):
        A.sddmm(f(300, 2, 4), f(199, 2, 4))
    with pytest.raises(ValueError, match='columns'):
        A.set_value(f(row.size, 2), layout='coo').matmul_heads(f(199, 2, 4))
    rowptr, colidx, _ = A.csr()
    with pytest.raises(RuntimeError, match='heads'):
        torch.ops.tsamd.sddmm_heads(None, rowptr, colidx, None, f(300, 2, 4), f(200, 3, 4), 1.0)
    with pytest.raises(RuntimeError, match='heads'):
        torch.ops.tsamd.spmm_heads(rowptr, colidx, None, f(row.size, 2), f(200, 3, 4), 300)
    with pytest.raises(RuntimeError, match='entries'):
        torch.ops.tsamd.spmm_heads(rowptr, colidx, None, f(row.size - 1, 3), f(200, 3, 4), 300)
    with pytest.raises(RuntimeError, match='float32, float64, float16 or bfloat16'):
        torch.ops.tsamd.spmm_heads(rowptr, colidx, None, None, f(200, 3, 4).long(), 300)
    with pytest.raises(RuntimeError, match='dtype'):
        torch.ops.tsamd.sddmm_heads(None, rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4).double(), 1.0)
