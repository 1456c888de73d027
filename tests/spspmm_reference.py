"""The comparators of the SpSpMM forward tests against the numpy oracle (oracle.np_oracle.spspmm fed float64 values), for
the cases of tests/spspmm_cases.py -- numpy only, no GPU.  tests/test_spspmm_reference.py holds them to the reference:
the oracle against torch.sparse.mm, and eight planted defects that they must reject.  Test infrastructure, not a conftest.

Criteria, the ones of tests/test_spspmm_wide_gpu.py (no other tolerance is used):
  indices, rowptr     bit-exact, always
  dyadic values       (non-zero half-integers: every sum exact) bit-equal
  cancelling rows     (case['cancel']: +v and -v over two identical rows of B) every value has the bits of +0.0
  uniform(-0.5, 0.5)  fp32: |got - ref64| <= 1e-5 * sum|terms| per entry
                      fp64: |got - ref64| <= 2 * (n + 1) * 2^-53 * sum|terms|, n = products of the entry
"""
import numpy as np

from oracle import np_oracle as no
from tests import spspmm_cases as sc


def bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def pattern_and_terms(case):
    """-> (row, col, products per entry, rowptr) of C: the oracle on all-ones operands.  Computed once per case."""
    if '_pattern' not in case:
        r, c, n = no.spspmm(case['rowA'], case['colA'], None, case['rowB'], case['colB'], None, case['m'], case['k'],
                            case['N'])
        rowptr = np.zeros(case['m'] + 1, np.int64)
        rowptr[1:] = np.cumsum(np.bincount(r, minlength=case['m']))
        for a in (r, c, n, rowptr):
            a.setflags(write=False)
        case['_pattern'] = (r, c, n, rowptr)
    return case['_pattern']


def apply_cancel(case, va, vb):
    """The cancelling rows of a narrow case: the second entry of A is minus the first, the second row of B repeats the
    values of the first.  Applied AFTER every replacement of zero values, so that the signs survive."""
    rpA, rpB = case['rowptrA'], case['rowptrB']
    for _, i, b1, b2 in case.get('cancel', ()):
        e = rpA[i]
        if va is not None:
            assert va[e] != 0
            va[e + 1] = -va[e]
        if vb is not None:
            vb[rpB[b2]:rpB[b2 + 1]] = vb[rpB[b1]:rpB[b1 + 1]]


def make_values(case, np_dtype, mode, kind):
    """-> (valA, valB) in the value type (None where the operand has no values)."""
    va, vb = sc.values(case, kind)
    if kind == 'dyadic':  # no zeros: a product of -0.0 would make "bit-equal" a statement about signed zeros
        va[va == 0] = 0.5
        vb[vb == 0] = -1.5
    va = va.astype(np_dtype) if mode in ('both', 'a_only') else None
    vb = vb.astype(np_dtype) if mode in ('both', 'b_only') else None
    apply_cancel(case, va, vb)
    return va, vb


def reference(case, va, vb):
    """-> (ref, l1): the float64 product and sum|terms| per entry of C."""
    f64 = lambda a: None if a is None else a.astype(np.float64)  # noqa: E731
    ab = lambda a: None if a is None else np.abs(a.astype(np.float64))  # noqa: E731
    args = (case['m'], case['k'], case['N'])
    _, _, ref = no.spspmm(case['rowA'], case['colA'], f64(va), case['rowB'], case['colB'], f64(vb), *args)
    _, _, l1 = no.spspmm(case['rowA'], case['colA'], ab(va), case['rowB'], case['colB'], ab(vb), *args)
    return ref, l1


def bound(np_dtype, n, l1):
    return 1e-5 * l1 if np_dtype == np.float32 else 2.0 * (n + 1.0) * 2.0 ** -53 * l1


def check_pattern(case, rpC, cC):
    r, c, n, rowptr = pattern_and_terms(case)
    assert rpC.dtype == np.int64 and cC.dtype == np.int64
    assert np.array_equal(rpC, rowptr), 'rowptr of C'
    assert np.array_equal(cC, c), 'column ids of C'
    assert int(c.max()) == case['N'] - 1  # the last valid column id is part of the result


def check_values(case, np_dtype, va, vb, kind, vC, ref_l1=None):
    """-> largest |got - ref| / sum|terms| over the entries."""
    ref, l1 = reference(case, va, vb) if ref_l1 is None else ref_l1
    _, _, n, rowptr = pattern_and_terms(case)
    assert vC.dtype == np_dtype and vC.shape == ref.shape
    err = np.abs(vC.astype(np.float64) - ref)
    ratio = float((err / np.maximum(l1, 1e-300)).max())
    if kind == 'dyadic':
        want = ref.astype(np_dtype)
        assert np.array_equal(want.astype(np.float64), ref)  # the reference itself is exact in the value type
        assert np.array_equal(bits(vC), bits(want)), 'dyadic values: not bit-equal'
    elif np_dtype == np.float32:
        bad = err > bound(np_dtype, n, l1)
        assert not bad.any(), 'fp32: %d entries beyond 1e-5 * sum|terms| (worst ratio %.3e)' % (int(bad.sum()), ratio)
    else:
        bad = err > bound(np_dtype, n, l1)
        assert not bad.any(), 'fp64: %d entries beyond 2 (n + 1) 2^-53 * sum|terms| (worst ratio %.3e)' % (
            int(bad.sum()), ratio)
    if va is not None:  # an exact zero is an entry, and it is +0.0: x + (-x) in round-to-nearest
        for name, i, _, _ in case.get('cancel', ()):
            s, e = rowptr[i], rowptr[i + 1]
            assert e > s and bool((bits(vC[s:e]) == 0).all()), '%s: not every value has the bits of +0.0' % name
    return ratio


def check_row(case, np_dtype, name, rpC, cC, vC, ref, l1):
    """One named row against the reference, so that a failure names the row."""
    r, c, n, rowptr = pattern_and_terms(case)
    i = case['names'].index(name)
    s, e = int(rowptr[i]), int(rowptr[i + 1])
    assert e > s, name
    assert (int(rpC[i]), int(rpC[i + 1])) == (s, e), '%s: rowptr' % name
    assert np.array_equal(cC[s:e], c[s:e]), '%s: column ids' % name
    err = np.abs(vC[s:e].astype(np.float64) - ref[s:e])
    assert bool((err <= bound(np_dtype, n[s:e], l1[s:e])).all()), '%s (%d products): worst ratio %.3e' % (
        name, int(case['census']['products'][i]), float((err / np.maximum(l1[s:e], 1e-300)).max()))


# ---- rows of the oracle's own result, for the planted defects of tests/test_spspmm_reference.py ----------------------
def row_terms(case, i, va, vb):
    """(columns, products) of row i in expansion order, products in float64."""
    rpA, rpB = case['rowptrA'], case['rowptrB']
    cols, vals = [], []
    for e in range(rpA[i], rpA[i + 1]):
        kk = case['colA'][e]
        s, t = rpB[kk], rpB[kk + 1]
        cols.append(case['colB'][s:t])
        a = 1.0 if va is None else float(va[e])
        vals.append(a * (np.ones(t - s) if vb is None else vb[s:t].astype(np.float64)))
    if not cols:
        return np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(cols), np.concatenate(vals)


def sorted_terms(cols, vals):
    perm = np.argsort(cols, kind='stable')
    return cols[perm], vals[perm]


def sum_runs(cols, vals):
    """Sorted terms -> (distinct columns, sums)."""
    head = np.ones(cols.size, bool)
    head[1:] = cols[1:] != cols[:-1]
    starts = np.nonzero(head)[0]
    return cols[head], (np.add.reduceat(vals, starts) if cols.size else vals[:0])


def splice_row(rowptr, col, val, i, new_col, new_val):
    """The CSR result with row i replaced."""
    s, e = int(rowptr[i]), int(rowptr[i + 1])
    rp = rowptr.copy()
    rp[i + 1:] += new_col.size - (e - s)
    return rp, np.concatenate([col[:s], new_col, col[e:]]), np.concatenate([val[:s], new_val.astype(val.dtype), val[e:]])
