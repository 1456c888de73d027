"""The comparators of tests/spspmm_reference.py held to the reference, without a GPU: the numpy oracle against
torch.sparse.mm in float64, the census of every grid point of tests/test_spspmm_narrow_gpu.py, and eight planted
defects -- each applied to the oracle's own output -- that the comparators must reject while they accept the clean
output."""
import numpy as np
import pytest
import torch

from tests import spspmm_cases as sc
from tests import spspmm_reference as sr

LG = {'fp32': 13, 'fp64': 12}   # TSAMD_SPSPMM_LG_RANGE by value type (tests/test_spspmm_route.py pins it)
NP_DT = {'fp32': np.float32, 'fp64': np.float64}
GRID = [(dt, N) for dt in ('fp32', 'fp64') for N in sc.ordinary_grid(LG[dt])]
NARROW = [(dt, N) for dt in ('fp32', 'fp64') for N in sc.narrow_grid(LG[dt])]
gid = lambda g: ['%s-N%d' % p for p in g]  # noqa: E731


@pytest.mark.parametrize('N', [1, (1 << 13) + 1, 8 << 13])
def test_oracle_matches_torch_sparse_mm(N):
    """Pattern bit-exact (explicit zeros included), values within 2 (n + 1) 2^-53 sum|terms|: both sum n products in
    float64, in whatever order."""
    case = sc.grid_case(N, 13)
    va, vb = sr.make_values(case, np.float64, 'both', 'uniform')
    A = torch.sparse_coo_tensor(np.stack([case['rowA'], case['colA']]), va, (case['m'], case['k'])).coalesce()
    B = torch.sparse_coo_tensor(np.stack([case['rowB'], case['colB']]), vb, (case['k'], N)).coalesce()
    C = torch.sparse.mm(A, B).coalesce()
    r, c, n, rowptr = sr.pattern_and_terms(case)
    index, value = C.indices().numpy(), C.values().numpy()
    assert np.array_equal(index[0], r) and np.array_equal(index[1], c)
    ref, l1 = sr.reference(case, va, vb)
    assert bool((np.abs(value - ref) <= sr.bound(np.float64, n, l1)).all())
    for name, i, _, _ in case['cancel']:  # torch keeps the exact zeros too
        assert rowptr[i + 1] > rowptr[i] and bool((value[rowptr[i]:rowptr[i + 1]] == 0).all()), name
    assert n.sum() == case['census']['products'].sum()


@pytest.mark.parametrize('dt,N', GRID, ids=gid(GRID))
def test_grid_case_census(dt, N):
    case = sc.grid_case(N, LG[dt])
    sc.assert_census(case)
    r, c, n, rowptr = sr.pattern_and_terms(case)
    assert rowptr[-1] == c.size and int(n.sum()) == int(case['census']['products'].sum())


@pytest.mark.parametrize('dt,N', NARROW, ids=gid(NARROW))
def test_narrow_builder_is_deterministic_and_seeded(dt, N):
    lg = LG[dt]
    seed = 1 + sc.ordinary_grid(lg).index(N)
    case, again, other = sc.grid_case(N, lg), sc.make_narrow_case(N, lg, seed=seed), sc.make_narrow_case(N, lg, seed=99)
    assert case['seed'] == seed and case['names'] == again['names']
    for key in ('rowptrA', 'colA', 'rowptrB', 'colB'):
        assert np.array_equal(case[key], again[key]), key
    sc.assert_reaches_narrow_routes(other)
    if N > 2:  # (with one or two columns there is nothing to draw)
        assert not np.array_equal(case['colB'], other['colB'])


def test_narrow_generator_refuses_sixteen_ranges():
    with pytest.raises(AssertionError):
        sc.make_narrow_case(15 * 8192 + 1, 13)
    with pytest.raises(AssertionError):
        sc.make_case(15 * 8192, 13)


@pytest.mark.parametrize('dt', ['fp32', 'fp64'])
def test_every_named_row_is_in_the_grid(dt):
    seen = set()
    for N in sc.narrow_grid(LG[dt]):
        seen.update(sc.grid_case(N, LG[dt])['names'])
    want = ['empty_first', 'empty_middle', 'empty_last', 'only_empty_b', 'run_cross_64', 'run_cross_256', 'run_from_63',
            'run_from_255', 'one_column_512', 'one_column_1024', 'one_column_large', 'distinct_512', 'distinct_1024',
            'stride_512', 'dense_range', 'dense_tail', 'tail_one', 'cancel_small', 'cancel_medium', 'cancel_big_bin',
            'cancel_group', 'long_a_512', 'long_a_513', 'long_a_2000', 'long_a_third', 'one_long_b', 'mixed_bins',
            'small', 'medium']
    want += ['exact_%d' % p for p in sc.EXACT_P] + ['group_%d' % g for g in sc.GROUP_G]
    assert not [n for n in want if n not in seen]


def test_classify_bins_returns_the_sizes():
    bins = np.zeros(600, np.int64)
    bins[[0, 1, 2, 3, 300, 301]] = [600, 424, 1, 1025, 5, 6]
    assert sc.classify_bins(bins) == (1, 1, 0, 3, [1024, 1, 11], [1025])
    bins[301] = 0
    bins[599] = 7
    assert sc.classify_bins(bins) == (1, 1, 1, 4, [1024, 1, 5, 7], [1025])


# ---- planted defects -------------------------------------------------------------------------------------------------
def clean(dt, kind, N=None):
    """The case at N = R + 1 (every named row but dense_tail), its values and the oracle's own output."""
    lg = LG[dt]
    case = sc.grid_case((1 << lg) + 1 if N is None else N, lg)
    va, vb = sr.make_values(case, NP_DT[dt], 'both', kind)
    r, c, n, rowptr = sr.pattern_and_terms(case)
    ref, l1 = sr.reference(case, va, vb)
    return case, va, vb, rowptr.copy(), c.copy(), ref.astype(NP_DT[dt])


def full_check(case, dt, va, vb, kind, out):
    rp, c, v = out
    sr.check_pattern(case, rp, c)
    sr.check_values(case, NP_DT[dt], va, vb, kind, v)


def rejects(case, dt, va, vb, kind, out):
    with pytest.raises(AssertionError):
        full_check(case, dt, va, vb, kind, out)


def replace_row(case, name, out, new_col, new_val):
    return sr.splice_row(out[0], out[1], out[2], case['names'].index(name), np.asarray(new_col, np.int64),
                         np.asarray(new_val))


def row_slice(case, name, out):
    i = case['names'].index(name)
    return int(out[0][i]), int(out[0][i + 1])


KINDS = [(dt, kind) for dt in ('fp32', 'fp64') for kind in ('dyadic', 'uniform')]
kid = ['%s-%s' % p for p in KINDS]


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_comparators_accept_the_clean_output(dt, kind):
    for N in (None, 1, 15 * (1 << LG[dt]) - 3):
        case, va, vb, *out = clean(dt, kind, N)
        full_check(case, dt, va, vb, kind, out)
        for mode in ('a_only', 'b_only'):
            va1, vb1 = sr.make_values(case, NP_DT[dt], mode, kind)
            ref, _ = sr.reference(case, va1, vb1)
            sr.check_values(case, NP_DT[dt], va1, vb1, kind, ref.astype(NP_DT[dt]))


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_1_last_product_of_a_row_dropped(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name in ('exact_65', 'exact_1025', 'one_column_512'):
        cols, vals = sr.row_terms(case, case['names'].index(name), va, vb)
        rejects(case, dt, va, vb, kind, replace_row(case, name, out, *sr.sum_runs(*sr.sorted_terms(cols[:-1], vals[:-1]))))


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_2_two_equal_columns_left_unmerged(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name in ('exact_513', 'run_cross_64'):
        cols, vals = sr.sorted_terms(*sr.row_terms(case, case['names'].index(name), va, vb))
        j = int(np.nonzero(cols[1:] == cols[:-1])[0][0]) + 1  # the second term of the first run: it starts an entry
        c1, v1 = sr.sum_runs(cols[:j], vals[:j])
        c2, v2 = sr.sum_runs(cols[j:], vals[j:])
        bad = replace_row(case, name, out, np.concatenate([c1, c2]), np.concatenate([v1, v2]))
        assert bad[1].size == out[1].size + 1
        rejects(case, dt, va, vb, kind, bad)


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_3_two_neighbouring_columns_swapped(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name in ('exact_64', 'dense_range'):
        s, e = row_slice(case, name, out)
        rp, c, v = out[0], out[1].copy(), out[2].copy()
        j = (s + e) // 2
        c[[j, j + 1]] = c[[j + 1, j]]
        v[[j, j + 1]] = v[[j + 1, j]]
        rejects(case, dt, va, vb, kind, (rp, c, v))


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_4_an_exact_zero_entry_dropped(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name, i, _, _ in case['cancel']:
        s, e = row_slice(case, name, out)
        assert e - s >= 1 and bool((sr.bits(out[2][s:e]) == 0).all())
        j = (e - s) // 2
        rejects(case, dt, va, vb, kind, replace_row(case, name, out, np.delete(out[1][s:e], j), np.delete(out[2][s:e], j)))
    # ... and a zero that is there with the wrong sign
    s, e = row_slice(case, 'cancel_small', out)
    v = out[2].copy()
    v[s] = -0.0
    rejects(case, dt, va, vb, kind, (out[0], out[1], v))


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_5_entry_on_the_last_column_lost(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name in ('one_column_512', 'tail_one', 'one_column_large'):
        s, e = row_slice(case, name, out)
        assert out[1][e - 1] == case['N'] - 1
        rejects(case, dt, va, vb, kind, replace_row(case, name, out, out[1][s:e - 1], out[2][s:e - 1]))


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_6_value_moved_to_the_neighbouring_entry(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name in ('exact_129', 'distinct_1024', 'group_65'):
        s, e = row_slice(case, name, out)
        v = out[2].copy()
        j = s + int(np.nonzero(v[s:e - 1] != v[s + 1:e])[0][0])
        v[j + 1] += v[j]
        v[j] = 0
        rejects(case, dt, va, vb, kind, (out[0], out[1], v))
        v = out[2].copy()
        v[[j, j + 1]] = v[[j + 1, j]]
        rejects(case, dt, va, vb, kind, (out[0], out[1], v))


@pytest.mark.parametrize('dt,kind', KINDS, ids=kid)
def test_defect_7_run_summed_without_its_part_behind_position_64(dt, kind):
    case, va, vb, *out = clean(dt, kind)
    for name, cut in (('run_cross_64', 64), ('run_from_63', 64), ('run_cross_256', 256), ('run_from_255', 256)):
        cols, vals = sr.sorted_terms(*sr.row_terms(case, case['names'].index(name), va, vb))
        first, last, cnt = sc.run_positions(case, case['names'].index(name), case['run_col'])
        assert first < cut <= last
        keep = np.ones(cols.size, bool)
        keep[cut:last + 1] = False  # the head lane stops at the end of its chunk
        bad = replace_row(case, name, out, *sr.sum_runs(cols[keep], vals[keep]))
        assert np.array_equal(bad[1], out[1])
        rejects(case, dt, va, vb, kind, bad)


@pytest.mark.parametrize('dt', ['fp32', 'fp64'])
def test_defect_8_one_ulp_on_a_dyadic_value(dt):
    case, va, vb, *out = clean(dt, 'dyadic')
    for name in ('exact_1', 'exact_1024', 'one_column_large', 'cancel_group'):
        s, e = row_slice(case, name, out)
        for j in (s, e - 1):
            v = out[2].copy()
            v[j] = np.nextafter(v[j], NP_DT[dt](np.inf))
            rejects(case, dt, va, vb, 'dyadic', (out[0], out[1], v))
