"""SpSpMM at ordinary widths -- 1 to 2^22 columns in B, where config 4 (N = 500 000) and every everyday product run:
every route of csrc/spspmm.hip that a row can take there, against the numpy oracle fed float64 values.  Below 16 column
ranges the cases come from tests/spspmm_cases.make_narrow_case (named rows: the keys-per-lane ladder 64 / 128 / 256 /
512 / 1024 of the register sort for rows and for groups, runs of one column across the chunks of compress_and_store,
dense ranges, exact zeros, full hash sets, the count kernel's whole-wave path, one bin per large row at nr = 1);
from 16 ranges on from make_case.  Each test asserts the route (tsamd_spspmm_route, REGIMES below) and the host census of
its input before it looks at the GPU.

Criteria: tests/spspmm_reference.py (the ones of tests/test_spspmm_wide_gpu.py; tests/test_spspmm_reference.py holds them
to planted defects).  sub = 4 at every N of this grid: two runs are bit-identical, asserted unconditionally.

Every test prints a `NARROW-STAT` line (largest |gpu - ref| / sum|terms|) for -s runs.
"""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import spspmm_cases as sc
from tests import spspmm_reference as sr
from tests.spspmm_reference import bits

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
TORCH_DT = {F32: torch.float32, F64: torch.float64}
NP_DT = {F32: np.float32, F64: np.float64}
DT_NAME = {F32: 'fp32', F64: 'fp64'}
R32, R64 = 1 << 13, 1 << 12   # columns per range

# What the dispatch does at each N of the grid, written out (tests/test_spspmm_route.py pins the same rows):
# (dtype, N) -> (nr, sub, off_lds, small_pairs, passes, narrow_hash, large_ok).  Everywhere here: per-wave bin segments
# (sub 4, spspmm_large_accum_wave_kernel), segment offsets in LDS, the register sort for the small rows, the 24-bit hash
# multiply; only the number of ranges and the radix passes of the (unused) pairs sort move.
REGIMES = {
    (F32, 1): (1, 4, 1, 0, 1, 1, 1),
    (F32, 2): (1, 4, 1, 0, 1, 1, 1),
    (F32, 97): (1, 4, 1, 0, 1, 1, 1),
    (F32, R32): (1, 4, 1, 0, 2, 1, 1),
    (F32, R32 + 1): (2, 4, 1, 0, 2, 1, 1),
    (F32, 2 * R32): (2, 4, 1, 0, 2, 1, 1),
    (F32, 2 * R32 + 1): (3, 4, 1, 0, 2, 1, 1),
    (F32, 8 * R32): (8, 4, 1, 0, 2, 1, 1),
    (F32, 15 * R32 - 3): (15, 4, 1, 0, 3, 1, 1),
    (F32, 16 * R32): (16, 4, 1, 0, 3, 1, 1),
    (F32, 500000): (62, 4, 1, 0, 3, 1, 1),
    (F32, 1 << 21): (256, 4, 1, 0, 3, 1, 1),
    (F32, 1 << 22): (512, 4, 1, 0, 3, 1, 1),
    (F64, 1): (1, 4, 1, 0, 1, 1, 1),
    (F64, 2): (1, 4, 1, 0, 1, 1, 1),
    (F64, 97): (1, 4, 1, 0, 1, 1, 1),
    (F64, R64): (1, 4, 1, 0, 2, 1, 1),
    (F64, R64 + 1): (2, 4, 1, 0, 2, 1, 1),
    (F64, 2 * R64): (2, 4, 1, 0, 2, 1, 1),
    (F64, 2 * R64 + 1): (3, 4, 1, 0, 2, 1, 1),
    (F64, 8 * R64): (8, 4, 1, 0, 2, 1, 1),
    (F64, 15 * R64 - 3): (15, 4, 1, 0, 2, 1, 1),
    (F64, 16 * R64): (16, 4, 1, 0, 2, 1, 1),
    (F64, 500000): (123, 4, 1, 0, 3, 1, 1),
    (F64, 1 << 21): (512, 4, 1, 0, 3, 1, 1),
    (F64, 1 << 22): (1024, 4, 1, 0, 3, 1, 1),
}
LG = {F32: 13, F64: 12}
GRID = [(dt, N) for dt in (F32, F64) for N in sc.ordinary_grid(LG[dt])]
assert sorted(GRID) == sorted(REGIMES)
VALUE_MODES = ['both', 'a_only', 'b_only', 'none']
# rows that a failure should name (those a case has; the census says which it must have)
NAMED = ['exact_%d' % p for p in sc.EXACT_P] + [
    'sentinel_512', 'run_cross_64', 'run_from_63', 'run_cross_256', 'run_from_255', 'one_column_512', 'one_column_1024',
    'one_column_large', 'distinct_512', 'distinct_1024', 'stride_512', 'dense_range', 'dense_tail', 'tail_one',
    'cancel_small', 'cancel_medium', 'cancel_big_bin', 'cancel_group', 'long_a_512', 'long_a_513', 'long_a_2000',
    'long_a_third', 'one_long_b', 'mixed_bins', 'cap_large', 'mixed_large'] + ['group_%d' % g for g in sc.GROUP_G]


def label(dtype, N):
    R = 1 << LG[dtype]
    for mult in (1, 2, 8, 15, 16):
        for d in (-3, 0, 1):
            if N == mult * R + d and N > 97:
                return '%s-N%sR%s-nr%d' % (DT_NAME[dtype], '' if mult == 1 else mult, '%+d' % d if d else '',
                                           REGIMES[(dtype, N)][0])
    return '%s-N%d-nr%d' % (DT_NAME[dtype], N, REGIMES[(dtype, N)][0])


def ids(grid):
    return [label(dt, N) for dt, N in grid]


def expect_route(dtype, N):
    """The regime this test was written for is the one the library takes: -> lg_range."""
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spspmm_route(dtype, ctypes.c_int64(N), out) == 0
    got = tuple(int(x) for x in out)
    assert got[1:] == REGIMES[(dtype, N)], (DT_NAME[dtype], N, got)
    assert got[0] == LG[dtype] and got[2] == 4 and got[7] == 1
    return got[0]


def get_case(dtype, N):
    """Route and census first, then the case."""
    case = sc.grid_case(N, expect_route(dtype, N))
    sc.assert_census(case)
    return case


def dev_operands(case, va, vb, dev):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return t(case['rowptrA']), t(case['colA']), t(va), t(case['rowptrB']), t(case['colB']), t(vb)


def run_op(case, va, vb, dev):
    rpA, cA, tva, rpB, cB, tvb = dev_operands(case, va, vb, dev)
    with_value = va is not None or vb is not None
    rpC, cC, vC = torch.ops.tsamd.spspmm(rpA, cA, tva, rpB, cB, tvb, case['N'], with_value)
    torch.cuda.synchronize()
    return rpC.cpu().numpy(), cC.cpu().numpy(), (vC.cpu().numpy() if with_value else None)


def run_functional(case, va, vb, dev):
    import pytorch_sparse_amd as ts
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    index, value = ts.spspmm(torch.stack([t(case['rowA']), t(case['colA'])]), t(va),
                             torch.stack([t(case['rowB']), t(case['colB'])]), t(vb), case['m'], case['k'], case['N'])
    return index.cpu().numpy(), (None if value is None else value.cpu().numpy())


def stat(test, dtype, N, mode, ratio):
    print('NARROW-STAT %s %s %s max|gpu-ref|/sum|terms|=%.3e' % (test, label(dtype, N), mode, ratio))


# ---- the C-ABI, stage by stage ---------------------------------------------------------------------------------------
i64, sz, vp = ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
ptr = lambda t: vp(0 if t is None else t.data_ptr())  # noqa: E731


def cabi_plan(case, dev):
    """tsamd_spspmm_plan -> dict(prod, bins, stats on the host; the device tensors for the later stages)."""
    L = nat.lib()
    rpA, cA, _, rpB, cB, _ = dev_operands(case, None, None, dev)
    M = case['m']
    opt = dict(dtype=torch.int64, device=dev)
    prod, bins, stats = torch.full((M + 1, ), -1, **opt), torch.full((2 * M + 1, ), -1, **opt), torch.empty(8, **opt)
    cB32 = torch.empty(cB.numel(), dtype=torch.int32, device=dev)
    assert L.tsamd_spspmm_plan(ptr(rpA), ptr(cA), ptr(rpB), ptr(cB), i64(cB.numel()), i64(M), ptr(prod), ptr(bins),
                               ptr(cB32), ptr(stats), nat.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    hs = stats.cpu().tolist()
    return dict(rpA=rpA, cA=cA, rpB=rpB, cB=cB, cB32=cB32, prod=prod, bins=bins, stats=hs, n_medium=hs[2], n_large=hs[3],
                P_large=hs[4])


def cabi_symbolic(case, dtype, plan, dev, tva=None, tvb=None, bin_values=0):
    """tsamd_spspmm_symbolic -> (per-row counts as written, before the scan; the workspace)."""
    L = nat.lib()
    M, N = case['m'], case['N']
    ws_bytes = L.tsamd_spspmm_workspace_bytes(dtype, i64(plan['n_large']), i64(plan['P_large']), i64(N))
    assert (ws_bytes > 0) == (plan['n_large'] > 0)
    ws = nat.workspace(ws_bytes, dev)
    rowptrC = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    assert L.tsamd_spspmm_symbolic(dtype, ptr(plan['rpA']), ptr(plan['cA']), ptr(tva), ptr(plan['rpB']),
                                   ptr(plan['cB32']), ptr(tvb), bin_values, i64(M), i64(N), ptr(plan['prod']),
                                   ptr(plan['bins']), i64(plan['n_medium']), i64(plan['n_large']), i64(plan['P_large']),
                                   ptr(rowptrC), ptr(ws), sz(ws.numel()), nat.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    return rowptrC, ws


def cabi_two_step(case, dtype, va, vb, dev):
    """plan -> symbolic WITHOUT values (bin_values = 0) -> scan -> numeric with values and values_binned = 0: what a C
    caller does that learns the values after the structure.  va = vb = None: structure only (valC = NULL)."""
    L = nat.lib()
    M, N = case['m'], case['N']
    plan = cabi_plan(case, dev)
    _, _, tva, _, _, tvb = dev_operands(case, va, vb, dev)
    rowptrC, ws = cabi_symbolic(case, dtype, plan, dev)
    stream = nat.stream_ptr(dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws2 = nat.workspace(L.tsamd_exclusive_scan_workspace_bytes(i64(M + 1)), dev)
    assert L.tsamd_exclusive_scan_i64(ptr(rowptrC), ptr(rowptrC), i64(M + 1), ptr(total), ptr(ws2), sz(ws2.numel()),
                                      stream) == 0
    nnz = int(total.item())
    colC = torch.empty(nnz, dtype=torch.int64, device=dev)
    valC = torch.empty(nnz, dtype=TORCH_DT[dtype], device=dev) if (va is not None or vb is not None) else None
    assert L.tsamd_spspmm_numeric(dtype, ptr(plan['rpA']), ptr(plan['cA']), ptr(tva), ptr(plan['rpB']), ptr(plan['cB32']),
                                  ptr(tvb), i64(M), i64(N), ptr(plan['prod']), ptr(plan['bins']), i64(plan['n_medium']),
                                  i64(plan['n_large']), i64(plan['P_large']), ptr(rowptrC), ptr(colC), ptr(valC), 0,
                                  ptr(ws), sz(ws.numel()), stream) == 0
    torch.cuda.synchronize()
    return rowptrC.cpu().numpy(), colC.cpu().numpy(), (None if valC is None else valC.cpu().numpy())


# ---- tests -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', VALUE_MODES)
@pytest.mark.parametrize('dtype,N', GRID, ids=ids(GRID))
def test_narrow_product_matches_oracle(dev, dtype, N, mode):
    """The whole case through torch.ops.tsamd.spspmm and the functional spspmm on its COO form: pattern bit-exact, dyadic
    values bit-equal (exact zeros: +0.0), rounding-sensitive values within the bound and bit-identical between two
    runs.  'a_only' / 'b_only': one operand without values; 'none': the value-less kernels (fp64: through the C-ABI --
    without values the op computes at the fp32 range width)."""
    case = get_case(dtype, N)
    npdt = NP_DT[dtype]
    r, c, _, _ = sr.pattern_and_terms(case)
    if mode == 'none':
        if dtype == F64:
            rpC, cC, vC = cabi_two_step(case, dtype, None, None, dev)
            assert vC is None
            sr.check_pattern(case, rpC, cC)
            rpC2, cC2, _ = cabi_two_step(case, dtype, None, None, dev)
            assert np.array_equal(rpC, rpC2) and np.array_equal(cC, cC2)
            return
        rpC, cC, vC = run_op(case, None, None, dev)
        assert vC is None
        sr.check_pattern(case, rpC, cC)
        index, value = run_functional(case, None, None, dev)
        assert value is None and np.array_equal(index[0], r) and np.array_equal(index[1], c)
        return

    va, vb = sr.make_values(case, npdt, mode, 'dyadic')
    rpC, cC, vC = run_op(case, va, vb, dev)
    sr.check_pattern(case, rpC, cC)
    sr.check_values(case, npdt, va, vb, 'dyadic', vC)
    index, value = run_functional(case, va, vb, dev)
    assert np.array_equal(index[0], r) and np.array_equal(index[1], c)
    assert np.array_equal(bits(value), bits(vC))

    va, vb = sr.make_values(case, npdt, mode, 'uniform')
    ref_l1 = sr.reference(case, va, vb)
    rpC, cC, vC = run_op(case, va, vb, dev)
    sr.check_pattern(case, rpC, cC)
    ratio = sr.check_values(case, npdt, va, vb, 'uniform', vC, ref_l1)
    stat('oracle', dtype, N, mode, ratio)
    rpC2, cC2, vC2 = run_op(case, va, vb, dev)
    assert np.array_equal(rpC, rpC2) and np.array_equal(cC, cC2)
    assert np.array_equal(bits(vC), bits(vC2)), 'values differ between two runs (sub = 4: reproducible)'


@pytest.mark.parametrize('dtype,N', GRID, ids=ids(GRID))
def test_narrow_named_rows_row_by_row(dev, dtype, N):
    """Rounding-sensitive values, one assertion per named row, so that a failure prints the name.  The cancelling rows:
    as many entries as the oracle has, every one with the bits of +0.0."""
    case = get_case(dtype, N)
    npdt = NP_DT[dtype]
    va, vb = sr.make_values(case, npdt, 'both', 'uniform')
    ref, l1 = sr.reference(case, va, vb)
    rpC, cC, vC = run_op(case, va, vb, dev)
    names = [n for n in NAMED if n in case['names']]
    assert len(names) >= 8
    for name in names:
        sr.check_row(case, npdt, name, rpC, cC, vC, ref, l1)
    _, c, n, rowptr = sr.pattern_and_terms(case)
    for name, i, b1, _ in case.get('cancel', ()):
        assert rpC[i + 1] - rpC[i] == rowptr[i + 1] - rowptr[i] == np.diff(case['rowptrB'])[b1], name
        assert bool((bits(vC[rpC[i]:rpC[i + 1]]) == 0).all()), '%s: a value that is not +0.0' % name
    # the filler rows as well, by name and index
    worst = 0.0
    for i, name in enumerate(case['names']):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        assert (int(rpC[i]), int(rpC[i + 1])) == (s, e) and np.array_equal(cC[s:e], c[s:e]), (name, i)
        if e > s:
            err = np.abs(vC[s:e].astype(np.float64) - ref[s:e])
            assert bool((err <= sr.bound(npdt, n[s:e], l1[s:e])).all()), (name, i)
            worst = max(worst, float((err / np.maximum(l1[s:e], 1e-300)).max()))
    stat('named_rows', dtype, N, 'both', worst)


@pytest.mark.parametrize('dtype,N', GRID, ids=ids(GRID))
def test_plan_counts_word_for_word(dev, dtype, N):
    """tsamd_spspmm_plan: prod[0..M) is the census' products per row (the eight-lane path and the whole-wave path of
    spspmm_count_kernel alike: long_a_512 / long_a_513 and three long rows inside one wave), stats holds n_medium,
    n_large, P_large and the largest row, the two lists hold exactly the census' rows."""
    case = get_case(dtype, N)
    c, M = case['census'], case['m']
    plan = cabi_plan(case, dev)
    prod = plan['prod'].cpu().numpy()
    for i in np.nonzero(prod[:M] != c['products'])[0]:
        raise AssertionError('products of row %d (%s): %d, census %d' % (i, case['names'][i], prod[i], c['products'][i]))
    large_rows = np.nonzero(c['products'] > sc.MEDIUM_CAP)[0]
    medium_rows = np.nonzero((c['products'] > sc.SMALL_CAP) & (c['products'] <= sc.MEDIUM_CAP))[0]
    assert (plan['n_medium'], plan['n_large']) == (c['n_medium'], c['n_large']) == (medium_rows.size, large_rows.size)
    assert plan['P_large'] == int(c['products'][large_rows].sum())
    assert plan['stats'][5] == int(c['products'][large_rows].max())
    bins = plan['bins'].cpu().numpy()
    assert sorted(bins[:plan['n_medium']].tolist()) == medium_rows.tolist()
    assert sorted(bins[M:M + plan['n_large']].tolist()) == large_rows.tolist()


SYMBOLIC = [(dt, N) for dt in (F32, F64) for N in (1, 1 << LG[dt], (1 << LG[dt]) + 1, 8 << LG[dt], 500000)]


@pytest.mark.parametrize('dtype,N', SYMBOLIC, ids=ids(SYMBOLIC))
def test_symbolic_counts_word_for_word(dev, dtype, N):
    """What tsamd_spspmm_symbolic writes into rowptrC before the scan: the distinct columns of every row -- the hash
    sets of the small and medium rows (distinct_512 / distinct_1024 / stride_512 fill them to one half), the bitmaps of
    the big bins and the hash sets of the groups."""
    case = get_case(dtype, N)
    _, _, _, rowptr = sr.pattern_and_terms(case)
    want = np.diff(rowptr)
    plan = cabi_plan(case, dev)
    counts, _ = cabi_symbolic(case, dtype, plan, dev)
    counts = counts.cpu().numpy()
    assert counts[case['m']] == 0
    for i in np.nonzero(counts[:case['m']] != want)[0]:
        raise AssertionError('distinct columns of row %d (%s, %d products): %d, oracle %d' % (
            i, case['names'][i], case['census']['products'][i], counts[i], want[i]))


TWO_STEP = [(dt, N) for dt in (F32, F64) for N in (1 << LG[dt], (1 << LG[dt]) + 1, 8 << LG[dt])]


@pytest.mark.parametrize('dtype,N', TWO_STEP, ids=ids(TWO_STEP))
def test_narrow_cabi_two_step(dev, dtype, N):
    """values_binned = 0 with valC != NULL: the numeric stage bins the large rows a second time, now with values -- the
    same order as the first time (sub = 4), so the result is bit-identical to the op's, which bins once."""
    case = get_case(dtype, N)
    npdt = NP_DT[dtype]
    va, vb = sr.make_values(case, npdt, 'both', 'uniform')
    rpC, cC, vC = cabi_two_step(case, dtype, va, vb, dev)
    sr.check_pattern(case, rpC, cC)
    ratio = sr.check_values(case, npdt, va, vb, 'uniform', vC)
    rpO, cO, vO = run_op(case, va, vb, dev)
    assert np.array_equal(rpC, rpO) and np.array_equal(cC, cO)
    assert np.array_equal(bits(vC), bits(vO)), 'two-step result differs from the op'
    stat('two_step', dtype, N, 'both', ratio)
    rpC, cC, vC = cabi_two_step(case, dtype, va, None, dev)  # one operand without values through the same sequence
    sr.check_pattern(case, rpC, cC)
    sr.check_values(case, npdt, va, None, 'uniform', vC)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_narrow_sparse_tensor_matmul(dev, dtype):
    """SparseTensor @ SparseTensor at N = R + 1 and at config 4's width: CSR in, CSR out; the value-less product; the
    functional spspmm on a shuffled COO of the same operands (coalesced=True sorts them first): the same bits."""
    import pytorch_sparse_amd as ts
    npdt = NP_DT[dtype]
    for N in ((1 << LG[dtype]) + 1, 500000):
        case = get_case(dtype, N)
        m, k = case['m'], case['k']
        va, vb = sr.make_values(case, npdt, 'both', 'uniform')
        rpA, cA, tva, rpB, cB, tvb = dev_operands(case, va, vb, dev)
        A = ts.SparseTensor(rowptr=rpA, col=cA, value=tva, sparse_sizes=(m, k), is_sorted=True, trust_data=True)
        B = ts.SparseTensor(rowptr=rpB, col=cB, value=tvb, sparse_sizes=(k, N), is_sorted=True, trust_data=True)
        C = A @ B
        assert C.sparse_sizes() == (m, N)
        rpC, cC, vC = (t.cpu().numpy() for t in (C.storage.rowptr(), C.storage.col(), C.storage.value()))
        sr.check_pattern(case, rpC, cC)
        ratio = sr.check_values(case, npdt, va, vb, 'uniform', vC)
        r, c, _, _ = sr.pattern_and_terms(case)
        assert np.array_equal(C.storage.row().cpu().numpy(), r)
        stat('sparse_tensor', dtype, N, 'both', ratio)
        C0 = A.set_value(None, 'coo') @ B.set_value(None, 'coo')
        assert C0.storage.value() is None
        sr.check_pattern(case, C0.storage.rowptr().cpu().numpy(), C0.storage.col().cpu().numpy())
        rng = np.random.default_rng([dtype, N])
        pa, pb = rng.permutation(case['colA'].size), rng.permutation(case['colB'].size)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        index, value = ts.spspmm(torch.stack([t(case['rowA'][pa]), t(case['colA'][pa])]), t(va[pa]),
                                 torch.stack([t(case['rowB'][pb]), t(case['colB'][pb])]), t(vb[pb]), m, k, N,
                                 coalesced=True)
        assert np.array_equal(index[0].cpu().numpy(), r) and np.array_equal(index[1].cpu().numpy(), c)
        assert np.array_equal(bits(value.cpu().numpy()), bits(vC))
