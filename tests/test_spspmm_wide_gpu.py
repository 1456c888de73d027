"""SpSpMM with more than 2^22 columns in B: every kernel route csrc/spspmm.hip chooses from N (see REGIMES below and
tests/test_spspmm_route.py) against the numpy oracle fed float64 values, on the seeded hypersparse products of
tests/spspmm_cases.py (small, medium and large rows, exact class edges, bins above and below 1024 products, groups
closed by span and by the product cap).  Each test names the route it expects in its id, asserts it through
tsamd_spspmm_route and asserts the host census of its input before it looks at the GPU.

Criteria (no other tolerance is used):
  indices, rowptr     bit-exact, always
  dyadic values       (non-zero half-integers: every sum exact) bit-equal
  uniform(-0.5, 0.5)  fp32: |gpu - ref64| <= 1e-5 * sum|terms| per entry (as in
                      test_api_gpu.py::test_spspmm_values_are_reproducible_run_to_run);
                      fp64: |gpu - ref64| <= 2 * (n + 1) * 2^-53 * sum|terms|, n = products of the entry (one product
                      rounding + n - 1 additions on each side; the oracle sums in fp64 too)
  run to run          bit-identical where the large rows keep per-wave bin segments (sub = 4) or there are no large
                      rows; with shared cursors (sub = 1: N > 2^24 fp32, N > 2^23 fp64) only the bounds are asserted

Every test prints a `WIDE-STAT` line (largest |gpu - ref| / sum|terms|, and whether two runs differed) for -s runs.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import np_oracle as no
from pytorch_sparse_amd import _native as nat
from tests import spspmm_cases as sc

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
TORCH_DT = {F32: torch.float32, F64: torch.float64}
NP_DT = {F32: np.float32, F64: np.float64}
DT_NAME = {F32: 'fp32', F64: 'fp64'}
P2 = lambda e, d=0: (1 << e) + d  # noqa: E731

# What the dispatch does at each N of the grid, written out (tests/test_spspmm_route.py pins the same thresholds):
# (dtype, N) -> (nr, sub, off_lds, small_pairs, passes, narrow_hash, large_ok)
#   sub 4 / 1      hist + bin kernels with per-wave segments, spspmm_large_accum_wave_kernel (one wave per big bin) /
#                  shared cursors, spspmm_large_accum_kernel (256-thread persistent accumulation)
#   off_lds 1 / 0  bin kernel: segment offsets in LDS / read from global memory
#   pairs 0 / 1    small rows: spspmm_numeric_small_kernel (register sort) / spspmm_numeric_pairs_kernel<T,64,512>
#                  (wave_radix_sort_lds) with `passes` radix passes
#   narrow 1 / 0   spspmm_symbolic_kernel<.., NARROW = true / false>, 64- and 256-thread forms
REGIMES = {
    (F32, P2(22, 1)): (513, 4, 1, 0, 3, 1, 1),
    (F32, P2(23)): (1024, 4, 1, 0, 3, 1, 1),
    (F32, P2(23, 1)): (1025, 4, 0, 1, 3, 1, 1),
    (F32, P2(24)): (2048, 4, 0, 1, 3, 1, 1),
    (F32, P2(24, 1)): (2049, 1, 1, 1, 4, 0, 1),
    (F32, P2(25)): (4096, 1, 1, 1, 4, 0, 1),
    (F32, P2(25, 1)): (4097, 1, 0, 1, 4, 0, 1),
    (F32, P2(26)): (8192, 1, 0, 1, 4, 0, 1),
    (F32, P2(26, 1)): (8193, 1, 0, 1, 4, 0, 0),
    (F32, P2(32, -2)): (1 << 19, 1, 0, 1, 4, 0, 0),
    (F64, P2(22, 1)): (1025, 4, 0, 0, 3, 1, 1),
    (F64, P2(23)): (2048, 4, 0, 0, 3, 1, 1),
    (F64, P2(23, 1)): (2049, 1, 1, 1, 3, 1, 1),
    (F64, P2(24)): (4096, 1, 1, 1, 3, 1, 1),
    (F64, P2(24, 1)): (4097, 1, 0, 1, 4, 0, 1),
    (F64, P2(25)): (8192, 1, 0, 1, 4, 0, 1),
    (F64, P2(25, 1)): (8193, 1, 0, 1, 4, 0, 0),
    (F64, P2(26)): (1 << 14, 1, 0, 1, 4, 0, 0),
    (F64, P2(26, 1)): ((1 << 14) + 1, 1, 0, 1, 4, 0, 0),
    (F64, P2(32, -2)): (1 << 20, 1, 0, 1, 4, 0, 0),
}
GRID_N = [P2(22, 1), P2(23), P2(23, 1), P2(24), P2(24, 1), P2(25), P2(25, 1), P2(26)]
NO_LARGE_N = [P2(26, 1), P2(32, -2)]
VALUE_MODES = ['both', 'a_only', 'b_only', 'none']


def n_label(N):
    for e in range(20, 33):
        for d in (-2, -1, 0, 1):
            if N == (1 << e) + d:
                return '2^%d%s' % (e, '%+d' % d if d else '')
    return str(N)


def regime_label(dtype, N):
    nr, sub, off, pairs, passes, narrow, ok = REGIMES[(dtype, N)]
    return '-'.join([DT_NAME[dtype], 'N' + n_label(N), 'sub%d' % sub if ok else 'nolarge',
                     'offlds' if off else 'offglobal', 'pairs_radix%d' % passes if pairs else 'regsort',
                     'hash24' if narrow else 'hash32'])


def route(dtype, N):
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spspmm_route(dtype, ctypes.c_int64(N), out) == 0
    return tuple(int(x) for x in out)


def expect_route(dtype, N):
    """The regime this test was written for is the one the library takes: -> (lg_range, sub, large_ok)."""
    got = route(dtype, N)
    assert got[1:] == REGIMES[(dtype, N)], (DT_NAME[dtype], N, got)
    return got[0], got[2], bool(got[7])


@functools.lru_cache(maxsize=None)
def get_case(N, lg_range, large):
    return sc.make_case(N, lg_range, seed=0, large=large)


@functools.lru_cache(maxsize=None)
def term_counts(N, lg_range, large):
    """Products per entry of C (the oracle on all-ones operands) and the rowptr of C."""
    case = get_case(N, lg_range, large)
    r, c, n = no.spspmm(case['rowA'], case['colA'], None, case['rowB'], case['colB'], None, case['m'], case['k'], N)
    rowptr = np.zeros(case['m'] + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=case['m']))
    return r, c, n, rowptr


def make_values(case, dtype, mode, kind):
    """-> (valA, valB) in the value type (None where the operand has no values)."""
    va, vb = sc.values(case, kind)
    if kind == 'dyadic':  # no zeros: a product of -0.0 would make "bit-equal" a statement about signed zeros
        va[va == 0] = 0.5
        vb[vb == 0] = -1.5
    va = va.astype(NP_DT[dtype]) if mode in ('both', 'a_only') else None
    vb = vb.astype(NP_DT[dtype]) if mode in ('both', 'b_only') else None
    return va, vb


def dev_operands(case, va, vb, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return t(case['rowptrA']), t(case['colA']), t(va), t(case['rowptrB']), t(case['colB']), t(vb)


def run_op(case, va, vb, dev, n=None):
    rpA, cA, tva, rpB, cB, tvb = dev_operands(case, va, vb, dev)
    with_value = va is not None or vb is not None
    rpC, cC, vC = torch.ops.tsamd.spspmm(rpA, cA, tva, rpB, cB, tvb, case['N'] if n is None else n, with_value)
    torch.cuda.synchronize()
    return rpC.cpu().numpy(), cC.cpu().numpy(), (vC.cpu().numpy() if with_value else None)


def check_pattern(case, large, rpC, cC):
    r, c, n, rowptr = term_counts(case['N'], case['lg_range'], large)
    assert rpC.dtype == np.int64 and cC.dtype == np.int64
    assert np.array_equal(rpC, rowptr), 'rowptr of C'
    assert np.array_equal(cC, c), 'column ids of C'
    assert int(c.max()) == case['N'] - 1  # the last valid column id is part of the result


def check_values(case, large, dtype, va, vb, kind, vC):
    """-> largest |gpu - ref| / sum|terms| over the entries."""
    N, m, k = case['N'], case['m'], case['k']
    f64 = lambda a: None if a is None else a.astype(np.float64)  # noqa: E731
    ab = lambda a: None if a is None else np.abs(a.astype(np.float64))  # noqa: E731
    _, _, ref = no.spspmm(case['rowA'], case['colA'], f64(va), case['rowB'], case['colB'], f64(vb), m, k, N)
    _, _, l1 = no.spspmm(case['rowA'], case['colA'], ab(va), case['rowB'], case['colB'], ab(vb), m, k, N)
    _, _, n, _ = term_counts(N, case['lg_range'], large)
    assert vC.dtype == NP_DT[dtype] and vC.shape == ref.shape
    err = np.abs(vC.astype(np.float64) - ref)
    ratio = float((err / np.maximum(l1, 1e-300)).max())
    if kind == 'dyadic':
        want = ref.astype(NP_DT[dtype])
        assert np.array_equal(want.astype(np.float64), ref)  # the reference itself is exact in the value type
        assert np.array_equal(vC.view(np.int32 if dtype == F32 else np.int64),
                              want.view(np.int32 if dtype == F32 else np.int64)), 'dyadic values: not bit-equal'
    elif dtype == F32:
        bad = err > 1e-5 * l1
        assert not bad.any(), 'fp32: %d entries beyond 1e-5 * sum|terms| (worst ratio %.3e)' % (int(bad.sum()), ratio)
    else:
        bad = err > 2.0 * (n + 1.0) * 2.0 ** -53 * l1
        assert not bad.any(), 'fp64: %d entries beyond 2 (n + 1) 2^-53 * sum|terms| (worst ratio %.3e)' % (
            int(bad.sum()), ratio)
    return ratio


def bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def stat(test, dtype, N, mode, ratio, differed):
    print('WIDE-STAT %s %s %s max|gpu-ref|/sum|terms|=%.3e runs_differed=%s' % (
        test, regime_label(dtype, N), mode, ratio, differed))


GRID = [(dt, N) for dt in (F32, F64) for N in GRID_N]


@pytest.mark.parametrize('mode', VALUE_MODES)
@pytest.mark.parametrize('dtype,N', GRID, ids=[regime_label(dt, N) for dt, N in GRID])
def test_wide_product_matches_oracle(dev, dtype, N, mode):
    """The whole case (large rows wherever the regime supports them) through torch.ops.tsamd.spspmm and the
    functional spspmm: pattern bit-exact; dyadic values bit-equal; rounding-sensitive values within the bound, and
    bit-identical between two runs wherever the route is reproducible.  mode 'a_only' / 'b_only': one operand without
    values (valA / valB NULL inside kernels compiled WITH_VAL); 'none': the value-less kernels, large rows through
    spspmm_large_bin_kernel<T, false>."""
    import pytorch_sparse_amd as ts
    lg, sub, large_ok = expect_route(dtype, N)
    large = 'all' if large_ok else 'none'
    case = get_case(N, lg, large)
    census = case['census']
    if large_ok:
        sc.assert_reaches_every_route(case)  # small / medium / large rows, a bin > 1024, span and cap closures
    else:
        assert census['n_large'] == 0 and census['n_medium'] >= 1 and census['n_small'] >= 1
    reproducible = sub == 4 or not large_ok

    if mode == 'none':
        if dtype == F64:
            # without values the op (like the reference) computes in fp32; the value-less kernels at the fp64 range
            # width are what a C-ABI caller with dtype = TSAMD_F64 and valC = NULL gets
            rpC, cC, vC = cabi_two_step(case, dtype, None, None, dev)
            assert vC is None
            check_pattern(case, large, rpC, cC)
            stat('oracle', dtype, N, mode, 0.0, False)
            return
        rpC, cC, vC = run_op(case, None, None, dev)
        assert vC is None
        check_pattern(case, large, rpC, cC)
        t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        index, value = ts.spspmm(torch.stack([t(case['rowA']), t(case['colA'])]), None,
                                 torch.stack([t(case['rowB']), t(case['colB'])]), None, case['m'], case['k'], N)
        assert value is None
        r, c, _, _ = term_counts(N, lg, large)
        assert np.array_equal(index[0].cpu().numpy(), r) and np.array_equal(index[1].cpu().numpy(), c)
        stat('oracle', dtype, N, mode, 0.0, False)
        return

    va, vb = make_values(case, dtype, mode, 'dyadic')
    rpC, cC, vC = run_op(case, va, vb, dev)
    check_pattern(case, large, rpC, cC)
    check_values(case, large, dtype, va, vb, 'dyadic', vC)
    # the functional API on the COO form of the same operands: the same result
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    index, value = ts.spspmm(torch.stack([t(case['rowA']), t(case['colA'])]), t(va),
                             torch.stack([t(case['rowB']), t(case['colB'])]), t(vb), case['m'], case['k'], N)
    r, c, _, _ = term_counts(N, lg, large)
    assert np.array_equal(index[0].cpu().numpy(), r) and np.array_equal(index[1].cpu().numpy(), c)
    assert np.array_equal(bits(value.cpu().numpy()), bits(vC))

    va, vb = make_values(case, dtype, mode, 'uniform')
    rpC, cC, vC = run_op(case, va, vb, dev)
    check_pattern(case, large, rpC, cC)
    ratio = check_values(case, large, dtype, va, vb, 'uniform', vC)
    rpC2, cC2, vC2 = run_op(case, va, vb, dev)
    assert np.array_equal(rpC, rpC2) and np.array_equal(cC, cC2)
    ratio = max(ratio, check_values(case, large, dtype, va, vb, 'uniform', vC2))
    differed = not np.array_equal(bits(vC), bits(vC2))
    if reproducible:
        assert not differed, 'values differ between two runs on a route documented as reproducible'
    stat('oracle', dtype, N, mode, ratio, differed)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_wide_class_edges_row_by_row(dev, dtype):
    """The class edges, named: the rows of exactly 1 / 64 / 65 / 512 / 513 / 1024 / 1025 products and the 512-product
    row whose last key is (2^23 - 1) << 9 | 511 = the padding sentinel, with rounding-sensitive values at N = 2^23
    (register sort) and N = 2^23 + 1 (pairs radix sort) -- row by row, so that a failure names the row."""
    for N in (P2(23), P2(23, 1)):
        lg, sub, large_ok = expect_route(dtype, N)
        case = get_case(N, lg, 'all')
        names, prod = case['names'], case['census']['products']
        va, vb = make_values(case, dtype, 'both', 'uniform')
        rpC, cC, vC = run_op(case, va, vb, dev)
        check_pattern(case, 'all', rpC, cC)
        f64 = lambda a: a.astype(np.float64)  # noqa: E731
        r, c, ref = no.spspmm(case['rowA'], case['colA'], f64(va), case['rowB'], case['colB'], f64(vb), case['m'],
                              case['k'], N)
        _, _, l1 = no.spspmm(case['rowA'], case['colA'], np.abs(f64(va)), case['rowB'], case['colB'], np.abs(f64(vb)),
                             case['m'], case['k'], N)
        _, _, n, rowptr = term_counts(N, lg, 'all')
        for name in ['exact_%d' % p for p in (1, 64, 65, 512, 513, 1024, 1025)] + ['sentinel_512']:
            i = names.index(name)
            s, e = rowptr[i], rowptr[i + 1]
            assert e > s
            err = np.abs(vC[s:e].astype(np.float64) - ref[s:e])
            bound = 1e-5 * l1[s:e] if dtype == F32 else 2.0 * (n[s:e] + 1.0) * 2.0 ** -53 * l1[s:e]
            assert bool((err <= bound).all()), (name, int(prod[i]), n_label(N))
        s = names.index('sentinel_512')
        assert cC[rowptr[s + 1] - 1] == N - 1


NO_LARGE = [(dt, N) for dt in (F32, F64) for N in NO_LARGE_N]


@pytest.mark.parametrize('dtype,N', NO_LARGE, ids=[regime_label(dt, N) for dt, N in NO_LARGE])
def test_wide_beyond_the_large_row_limit_small_and_medium_rows_work(dev, dtype, N):
    """More column ranges than the large-row path supports, no large row: the 4-pass radix sort, the 32-bit-multiply
    hash and -- at N = 2^32 - 2 -- column id 2^32 - 3 next to the 0xFFFFFFFF sentinel / padding key."""
    lg, sub, large_ok = expect_route(dtype, N)
    assert not large_ok
    case = get_case(N, lg, 'none')
    c = case['census']
    assert c['n_large'] == 0 and c['n_medium'] >= 4 and c['n_small'] >= 10
    assert int(case['colB'].max()) == N - 1
    for kind in ('dyadic', 'uniform'):
        va, vb = make_values(case, dtype, 'both', kind)
        rpC, cC, vC = run_op(case, va, vb, dev)
        check_pattern(case, 'none', rpC, cC)
        ratio = check_values(case, 'none', dtype, va, vb, kind, vC)
        rpC2, cC2, vC2 = run_op(case, va, vb, dev)
        assert np.array_equal(cC, cC2) and np.array_equal(bits(vC), bits(vC2))
    stat('nolarge', dtype, N, 'both', ratio, False)
    rpC, cC, vC = run_op(case, None, None, dev)
    assert vC is None
    check_pattern(case, 'none', rpC, cC)


@pytest.mark.parametrize('dtype,N', [(F32, P2(26, 1)), (F64, P2(25, 1))], ids=['fp32-N2^26+1', 'fp64-N2^25+1'])
def test_wide_large_row_beyond_the_range_limit_is_refused(dev, dtype, N):
    """One large row with more than 8192 column ranges: tsamd_spspmm_symbolic answers TSAMD_ERR_UNSUPPORTED on the
    host (nothing of the large-row path is launched) and the op raises; the next ordinary product is correct."""
    lg, sub, large_ok = expect_route(dtype, N)
    assert not large_ok
    case = get_case(N, lg, 'one')
    assert case['census']['n_large'] == 1
    va, vb = make_values(case, dtype, 'both', 'dyadic')
    with pytest.raises(RuntimeError, match='tsamd_spspmm_symbolic'):
        run_op(case, va, vb, dev)
    if dtype == F32:  # (a value-less product is an fp32 product)
        with pytest.raises(RuntimeError, match='tsamd_spspmm_symbolic'):
            run_op(case, None, None, dev)
    torch.cuda.synchronize()
    N2 = P2(22, 1)
    lg2, _, ok2 = expect_route(dtype, N2)
    case2 = get_case(N2, lg2, 'all')
    va, vb = make_values(case2, dtype, 'both', 'dyadic')
    rpC, cC, vC = run_op(case2, va, vb, dev)
    check_pattern(case2, 'all', rpC, cC)
    check_values(case2, 'all', dtype, va, vb, 'dyadic', vC)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_wide_n_equal_to_the_sentinel_is_refused(dev, dtype):
    """N = 2^32 - 1 would allow column id 0xFFFFFFFF, the empty key of the hash sets: refused on the host."""
    N = P2(32, -2)
    lg, _, _ = expect_route(dtype, N)
    case = get_case(N, lg, 'none')
    va, vb = make_values(case, dtype, 'both', 'dyadic')
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spspmm_route(dtype, ctypes.c_int64(N + 1), out) == 2
    with pytest.raises(RuntimeError, match='tsamd_spspmm_symbolic'):
        run_op(case, va, vb, dev, n=N + 1)
    rpC, cC, vC = run_op(case, va, vb, dev)  # the same operands with N = 2^32 - 2 are fine
    check_pattern(case, 'none', rpC, cC)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_wide_sparse_tensor_matmul(dev, dtype):
    """SparseTensor @ SparseTensor at N = 2^24 + 1 (CSR in, CSR out: no colptr of 2^24 entries is ever built)."""
    import pytorch_sparse_amd as ts
    N = P2(24, 1)
    lg, sub, large_ok = expect_route(dtype, N)
    case = get_case(N, lg, 'all')
    sc.assert_reaches_every_route(case)
    va, vb = make_values(case, dtype, 'both', 'uniform')
    rpA, cA, tva, rpB, cB, tvb = dev_operands(case, va, vb, dev)
    A = ts.SparseTensor(rowptr=rpA, col=cA, value=tva, sparse_sizes=(case['m'], case['k']), is_sorted=True,
                        trust_data=True)
    B = ts.SparseTensor(rowptr=rpB, col=cB, value=tvb, sparse_sizes=(case['k'], N), is_sorted=True, trust_data=True)
    C = A @ B
    assert C.sparse_sizes() == (case['m'], N)
    check_pattern(case, 'all', C.storage.rowptr().cpu().numpy(), C.storage.col().cpu().numpy())
    ratio = check_values(case, 'all', dtype, va, vb, 'uniform', C.storage.value().cpu().numpy())
    r, _, _, _ = term_counts(N, lg, 'all')
    assert np.array_equal(C.storage.row().cpu().numpy(), r)
    stat('sparse_tensor', dtype, N, 'both', ratio, None)
    # value-less operands: a value-less result
    C0 = A.set_value(None, 'coo') @ B.set_value(None, 'coo')
    assert C0.storage.value() is None
    check_pattern(case, 'all', C0.storage.rowptr().cpu().numpy(), C0.storage.col().cpu().numpy())


def cabi_two_step(case, dtype, va, vb, dev):
    """plan -> symbolic WITHOUT values (bin_values = 0) -> scan -> numeric with values and values_binned = 0: what a
    C caller does that learns the values after the structure.  The large rows then go through a second
    spspmm_large_bin_kernel<T, true> launch inside the numeric stage.  va = vb = None: structure only (valC = NULL)."""
    L = nat.lib()
    i64, sz, vp = ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
    p = lambda t: vp(0 if t is None else t.data_ptr())  # noqa: E731
    rpA, cA, tva, rpB, cB, tvb = dev_operands(case, va, vb, dev)
    M, N = case['m'], case['N']
    stream = nat.stream_ptr(dev)
    i64opt = dict(dtype=torch.int64, device=dev)
    prod, bins, stats = torch.empty(M + 1, **i64opt), torch.empty(2 * M + 1, **i64opt), torch.empty(8, **i64opt)
    cB32 = torch.empty(cB.numel(), dtype=torch.int32, device=dev)
    assert L.tsamd_spspmm_plan(p(rpA), p(cA), p(rpB), p(cB), i64(cB.numel()), i64(M), p(prod), p(bins), p(cB32),
                               p(stats), stream) == 0
    hs = stats.cpu().tolist()
    n_medium, n_large, P_large = hs[2], hs[3], hs[4]
    c = case['census']
    assert (n_medium, n_large) == (c['n_medium'], c['n_large'])
    assert P_large == int(c['products'][c['products'] > sc.MEDIUM_CAP].sum())
    ws_bytes = L.tsamd_spspmm_workspace_bytes(dtype, i64(n_large), i64(P_large), i64(N))
    assert (ws_bytes > 0) == (n_large > 0)
    ws = nat.workspace(ws_bytes, dev)
    rowptrC = torch.zeros(M + 1, **i64opt)
    assert L.tsamd_spspmm_symbolic(dtype, p(rpA), p(cA), None, p(rpB), p(cB32), None, 0, i64(M), i64(N), p(prod),
                                   p(bins), i64(n_medium), i64(n_large), i64(P_large), p(rowptrC), p(ws),
                                   sz(ws.numel()), stream) == 0
    total = torch.empty(1, **i64opt)
    ws2 = nat.workspace(L.tsamd_exclusive_scan_workspace_bytes(i64(M + 1)), dev)
    assert L.tsamd_exclusive_scan_i64(p(rowptrC), p(rowptrC), i64(M + 1), p(total), p(ws2), sz(ws2.numel()),
                                      stream) == 0
    nnz = int(total.item())
    colC = torch.empty(nnz, **i64opt)
    valC = torch.empty(nnz, dtype=TORCH_DT[dtype], device=dev) if (va is not None or vb is not None) else None
    assert L.tsamd_spspmm_numeric(dtype, p(rpA), p(cA), p(tva), p(rpB), p(cB32), p(tvb), i64(M), i64(N), p(prod),
                                  p(bins), i64(n_medium), i64(n_large), i64(P_large), p(rowptrC), p(colC), p(valC),
                                  0, p(ws), sz(ws.numel()), stream) == 0
    torch.cuda.synchronize()
    return rowptrC.cpu().numpy(), colC.cpu().numpy(), (None if valC is None else valC.cpu().numpy())


TWO_STEP = [(F32, P2(23, 1)), (F32, P2(24, 1)), (F64, P2(23)), (F64, P2(23, 1))]


@pytest.mark.parametrize('dtype,N', TWO_STEP, ids=[regime_label(dt, N) for dt, N in TWO_STEP])
def test_wide_cabi_two_step_values_after_structure(dev, dtype, N):
    """values_binned = 0 with valC != NULL in numeric_large.  sub = 4: the second binning lays the products out in the
    same order as the first, the result is bit-identical to the op's (which bins once, with values); sub = 1: within
    the bounds."""
    lg, sub, large_ok = expect_route(dtype, N)
    assert large_ok
    case = get_case(N, lg, 'all')
    sc.assert_reaches_every_route(case)
    va, vb = make_values(case, dtype, 'both', 'uniform')
    rpC, cC, vC = cabi_two_step(case, dtype, va, vb, dev)
    check_pattern(case, 'all', rpC, cC)
    ratio = check_values(case, 'all', dtype, va, vb, 'uniform', vC)
    rpO, cO, vO = run_op(case, va, vb, dev)
    assert np.array_equal(rpC, rpO) and np.array_equal(cC, cO)
    differed = not np.array_equal(bits(vC), bits(vO))
    if sub == 4:
        assert not differed, 'two-step result differs from the op on a reproducible route'
    stat('two_step', dtype, N, 'both', ratio, differed)
    # one operand without values through the same sequence
    rpC, cC, vC = cabi_two_step(case, dtype, va, None, dev)
    check_pattern(case, 'all', rpC, cC)
    check_values(case, 'all', dtype, va, None, 'uniform', vC)
