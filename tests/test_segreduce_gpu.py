"""csrc/segreduce.hip (tsamd_segment_reduce_balanced) against tests/segreduce_reference.py on every route of its two
kernels: through the C-ABI below the operator's size gate, through tsamd::segment_reduce on either side of the gate,
and through SparseTensor.sum / mean / min / max(dim) and coalesce.  The route census is asserted on the host before
anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import segreduce_reference as R
from tests.util import SUM_ATOL, SUM_TOL, bits_equal, fromnp, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16,
         'i32': torch.int32, 'i64': torch.int64}
CASES = R.cases()
R.assert_reaches_every_route(CASES)  # hard: a layout that stops reaching a route fails the collection
_REF = {}  # (layout, kind, dtype, reduce) -> what check_result compares with; computed once, never written to


@pytest.fixture(scope='module')
def ts(dev):
    import pytorch_sparse_amd
    return pytorch_sparse_amd


def _tol(dtype):
    return dict(sum_tol=SUM_TOL.get(TORCH[dtype]), sum_atol=SUM_ATOL.get(TORCH[dtype]))


def _expect(case, kind, dtype, reduce, value):
    key = (case.name, kind, dtype, reduce)
    if key not in _REF:
        _REF[key] = R.reference(value, None, case.ptr, case.nseg, reduce, dtype, kind)
    return _REF[key]


def _balanced(value, perm, ptr, nseg, E, reduce, dtype_code=None):
    """tsamd_segment_reduce_balanced through ctypes: no size gate in front of it."""
    L = nat.lib()
    L.tsamd_segment_reduce_balanced_workspace_bytes.restype = ctypes.c_size_t
    D = value.numel() // value.size(0)
    dt = nat.DTYPES[value.dtype] if dtype_code is None else dtype_code
    nb = L.tsamd_segment_reduce_balanced_workspace_bytes(dt, nat._i64(E), nat._i64(D))
    assert nb >= 4 * 256
    ws = nat.workspace(nb, value.device)
    out = torch.full((nseg, ) + tuple(value.shape[1:]), 85, dtype=value.dtype, device=value.device)
    with torch.cuda.device(value.device):
        st = L.tsamd_segment_reduce_balanced(dt, nat.REDUCES[reduce], nat._ptr(value), nat._ptr(perm), nat._ptr(ptr),
                                             nat._i64(nseg), nat._i64(E), nat._i64(D), nat._ptr(out), nat._ptr(ws),
                                             ctypes.c_size_t(ws.numel()), nat.stream_ptr(value.device))
    nat.check(st, 'tsamd_segment_reduce_balanced')
    return out


def _sequential(value, perm, ptr, nseg, reduce):
    """tsamd_segment_reduce: one thread per (segment, feature), the loop every implementation is pinned to."""
    D = value.numel() // value.size(0)
    out = torch.empty((nseg, ) + tuple(value.shape[1:]), dtype=value.dtype, device=value.device)
    with torch.cuda.device(value.device):
        st = nat.lib().tsamd_segment_reduce(nat.DTYPES[value.dtype], nat.REDUCES[reduce], nat._ptr(value),
                                            nat._ptr(perm), nat._ptr(ptr), nat._i64(nseg), nat._i64(D),
                                            nat._ptr(out), nat.stream_ptr(value.device))
    nat.check(st, 'tsamd_segment_reduce')
    return out


def _reduces(kind):
    return R.REDUCES if kind in ('integers', 'uniform') else ('min', 'max')


COMBOS = [(d, k) for d in R.FLOATS for k in R.KINDS] + [(d, 'integers') for d in R.INTS]


# ---- (a) the C-ABI, every layout -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,kind', COMBOS, ids=['%s-%s' % c for c in COMBOS])
def test_cabi_every_layout(dev, dtype, kind):
    """Every layout x perm in {None, random} x D in {1, 3} x the reductions the value kind has an expectation for.
    'integers': the bits of the exact result and of the sequential kernel.  'uniform' sum / mean: the project's
    SUM_TOL * L1 + SUM_ATOL.  min / max of any kind: the bits of the sequential loop (reference and kernel).  Every
    call is made twice into a pre-filled output and must return the same bits."""
    tdt = TORCH[dtype]
    rng = np.random.default_rng(7)
    worst = 0.0
    for case in CASES:
        ptr = torch.from_numpy(case.ptr).to(dev)
        perm_np = rng.permutation(case.E)
        perm = torch.from_numpy(perm_np).to(dev)
        for reduce in _reduces(kind):
            v3 = R.values(case, kind, dtype, reduce)
            want = _expect(case, kind, dtype, reduce, v3)
            shuffled = np.empty_like(v3)
            shuffled[perm_np] = v3
            plain, mixed = fromnp(v3, tdt).to(dev), fromnp(shuffled, tdt).to(dev)
            slow = _sequential(plain, None, ptr, case.nseg, reduce)
            for D in (3, 1):
                for value, p in ((plain, None), (mixed, perm)):
                    val = value if D == 3 else value[:, 0].contiguous()
                    got = _balanced(val, p, ptr, case.nseg, case.E, reduce)
                    again = _balanced(val, p, ptr, case.nseg, case.E, reduce)
                    what = (case.name, reduce, D, 'perm' if p is not None else 'plain')
                    assert bits_equal(got, again), ('not deterministic', ) + what
                    exp = want if D == 3 else tuple(w[:, 0] for w in want)
                    try:
                        worst = max(worst, R.check_result(tonp(got), None, None, case.ptr, case.nseg, reduce, dtype,
                                                          kind, expect=exp, **_tol(dtype)))
                    except AssertionError as exc:
                        raise AssertionError('%s: %s' % (what, exc)) from None
                    if kind == 'integers' or reduce in ('min', 'max'):
                        assert bits_equal(got, slow if D == 3 else slow[:, 0]), ('sequential kernel', ) + what
    print('%s %s: worst err / bound %.3g' % (dtype, kind, worst))


def test_cabi_small_integers_pinned_to_their_status(dev):
    """u8 / i8 / i16 have an element size but no instantiation of this kernel: the entry answers UNSUPPORTED."""
    case = CASES[-1]
    ptr = torch.from_numpy(case.ptr).to(dev)
    for tdt in (torch.uint8, torch.int8, torch.int16):
        value = torch.ones(case.E, dtype=tdt, device=dev)
        with pytest.raises(nat.TsamdError, match='tsamd_segment_reduce_balanced failed: unsupported dtype, reduction or size'):
            _balanced(value, None, ptr, case.nseg, case.E, 'sum')


# ---- (b) tsamd::segment_reduce on either side of its gate --------------------------------------------------------
@pytest.mark.parametrize('E', [32767, 32768])
def test_operator_on_either_side_of_the_gate(ts, dev, E):
    """balanced=True below 32768 entries is the sequential kernel, from 32768 on the balanced one: the same bits for
    small integers and for min / max, sums within the bound of each other (and of fp64)."""
    case = R.gate_case(E)
    assert int(np.diff(case.ptr).max()) == E - 1000 and (E >= 32768) == (case.E >= 32768)
    ptr = torch.from_numpy(case.ptr).to(dev)
    op = torch.ops.tsamd.segment_reduce
    for dtype in ('f32', 'bf16', 'f64', 'i64'):
        for kind in (R.KINDS if dtype == 'f32' else ('integers', 'uniform') if dtype in R.FLOATS else ('integers', )):
            for reduce in _reduces(kind):
                v = R.values(case, kind, dtype, reduce)
                value = fromnp(v, TORCH[dtype]).to(dev)
                fast = op(value, None, ptr, case.nseg, reduce, True)
                slow = op(value, None, ptr, case.nseg, reduce, False)
                R.check_result(tonp(fast), v, None, case.ptr, case.nseg, reduce, dtype, kind, **_tol(dtype))
                if kind == 'integers' or reduce in ('min', 'max'):
                    assert bits_equal(fast, slow), (dtype, kind, reduce)
                else:
                    _, l1 = R.reduce_exact(R.to_acc(v, dtype), None, case.ptr, case.nseg, reduce)
                    bound = SUM_TOL[TORCH[dtype]] * l1 + SUM_ATOL[TORCH[dtype]]
                    assert bool((np.abs(fast.double().cpu().numpy() - slow.double().cpu().numpy()) <= bound).all())


def test_operator_one_segment_of_int64_weights(dev):
    """The partitioner's call (ops_partition.cpp): the totals of n vertex weights as one segment [0, n]."""
    n = 40001
    w = np.random.default_rng(3).integers(1, 1 << 20, n)
    value = torch.from_numpy(w).to(dev)
    seg = torch.tensor([0, n], device=dev)
    for reduce, want in (('sum', int(w.sum())), ('min', int(w.min())), ('max', int(w.max()))):
        got = torch.ops.tsamd.segment_reduce(value, None, seg, 1, reduce, True)
        assert got.dtype == torch.int64 and got.tolist() == [want], reduce
        assert _balanced(value, None, seg, 1, n, reduce).tolist() == [want]


# ---- (c) the public API ------------------------------------------------------------------------------------------
def _crafted_matrix():
    """Rows = the segments of the 'ruler' and 'long_mid' layouts (not a random graph); the columns of a row are a
    random rotation of 0..len-1 spread over 70001 columns, so the CSC order is a real permutation of the CSR order."""
    a, b = CASES[0], [c for c in CASES if c.name == 'long_mid'][0]
    assert a.name == 'ruler'
    ptr = np.concatenate([a.ptr, b.ptr[1:] + a.E])
    case = R.Case('crafted', ptr, int(ptr[-1]), ptr.size - 1)
    lens = np.diff(ptr)
    rng = np.random.default_rng(11)
    ncols = 70001
    row = np.repeat(np.arange(case.nseg), lens)
    local = np.arange(case.E) - ptr[row]
    col = (local + rng.integers(0, ncols, case.nseg)[row]) % ncols
    order = np.lexsort((col, row))  # columns ascending inside every row
    col = col[order]
    csr2csc = np.lexsort((row, col))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=ncols))]).astype(np.int64)
    assert case.E >= 32768 and int(lens.max()) < ncols and not np.array_equal(csr2csc, np.arange(case.E))
    return case, row, col, ncols, colptr, csr2csc


@pytest.fixture(scope='module')
def crafted():
    return _crafted_matrix()


@pytest.mark.parametrize('kind', ['uniform', 'nan', 'signed_zero'])
def test_sparse_tensor_reductions_on_crafted_rows(ts, dev, crafted, kind):
    """A.sum / mean / min / max(dim) for dim 1 (rowptr) and dim 0 (colptr through csr2csc), fp32."""
    case, row, col, ncols, colptr, csr2csc = crafted
    rp, c = torch.from_numpy(case.ptr).to(dev), torch.from_numpy(col).to(dev)
    for reduce in _reduces(kind):
        v = R.values(case, kind, 'f32', reduce, D=1)[:, 0]
        A = ts.SparseTensor(rowptr=rp, col=c, value=torch.from_numpy(v).to(dev), sparse_sizes=(case.nseg, ncols),
                            is_sorted=True)
        assert bool(torch.equal(A.storage.colptr().cpu(), torch.from_numpy(colptr)))
        for dim, perm, ptr, n in ((1, None, case.ptr, case.nseg), (0, csr2csc, colptr, ncols)):
            got = getattr(A, reduce)(dim=dim)
            assert got.shape == (n, )
            try:
                R.check_result(tonp(got), v, perm, ptr, n, reduce, 'f32', kind, **_tol('f32'))
            except AssertionError as exc:
                raise AssertionError('dim=%d %s: %s' % (dim, reduce, exc)) from None


@pytest.mark.parametrize('reduce', ['min', 'max'])
def test_min_max_gradients_on_crafted_rows(ts, dev, crafted, reduce):
    """Tie-free fp64 values: the gradient reaches exactly the winner, as torch.scatter_reduce's autograd routes it.  The
    backward reduces int64 candidates with 'min' on the balanced route."""
    case, row, col, ncols, colptr, csr2csc = crafted
    v = np.random.default_rng(5).permutation(case.E).astype(np.float64) / case.E - 0.5
    rp, c = torch.from_numpy(case.ptr).to(dev), torch.from_numpy(col).to(dev)
    for dim, index, n in ((1, row, case.nseg), (0, col, ncols)):
        val = torch.from_numpy(v).to(dev).requires_grad_()
        A = ts.SparseTensor(rowptr=rp, col=c, value=val, sparse_sizes=(case.nseg, ncols), is_sorted=True)
        gout = torch.from_numpy(np.random.default_rng(6).standard_normal(n)).to(dev)
        getattr(A, reduce)(dim=dim).backward(gout)
        ref = torch.from_numpy(v).to(dev).requires_grad_()
        torch.zeros(n, dtype=torch.float64, device=dev).scatter_reduce(
            0, torch.from_numpy(index).to(dev), ref, 'a' + reduce, include_self=False).backward(gout)
        assert torch.equal(val.grad, ref.grad), dim


def test_coalesce_heavy_duplication_against_fp64(ts, dev):
    """Six distinct pairs in 200 000 entries: runs of 33 000 duplicates reduced on the balanced route, rounding-
    sensitive fp32 values, against fp64 within SUM_TOL * L1 (min / max: the exact element)."""
    rng = np.random.default_rng(9)
    nnz = 200_000
    row, col = rng.integers(0, 3, nnz), rng.integers(0, 2, nnz)
    val = rng.uniform(-1.0, 1.0, (nnz, 2)).astype(np.float32)
    key = row * 2 + col
    order = np.argsort(key, kind='stable')
    ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=6))]).astype(np.int64)
    assert nnz > 8 * 6 and int(np.diff(ptr).min()) > 64 * R.CHUNK
    index = torch.from_numpy(np.stack([row, col])).to(dev)
    for op in ('add', 'mean', 'min', 'max'):
        oi, ov = ts.coalesce(index, torch.from_numpy(val).to(dev), 3, 2, op=op)
        assert (oi[0] * 2 + oi[1]).tolist() == list(range(6))
        reduce = 'sum' if op == 'add' else op
        exact, l1 = R.reduce_exact(val, order, ptr, 6, reduce)
        got = ov.cpu().numpy()
        if reduce in ('min', 'max'):
            assert np.array_equal(got.astype(np.float64), exact), op
        else:
            R.check_result(got, val, order, ptr, 6, reduce, 'f32', 'uniform', **_tol('f32'))
