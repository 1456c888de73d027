"""tests/rcm_oracle.py -- the level-synchronous restatement of scipy's reverse Cuthill-McKee that csrc/rcm.hip follows --
against scipy itself, on the graphs of tests/rcm_cases.py and on random graphs with diagonals, isolated nodes and many
components.  CPU only."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import rcm_cases, rcm_oracle as ro


def scipy_perm(rowptr, col):
    n = rowptr.size - 1
    if n == 0:  # scipy refuses to build a 0 x 0 matrix from arrays; its ordering of nothing is nothing
        return np.zeros(0, np.int64)
    A = sp.csr_matrix((np.ones(col.size, np.float32), col, rowptr), shape=(n, n))
    return sp.csgraph.reverse_cuthill_mckee(A, symmetric_mode=True).astype(np.int64)


def random_graph(rng, n):
    """A symmetric graph on n nodes with about n / 4 nodes left isolated, a few diagonals, several components."""
    m = int(rng.integers(0, 2 * n + 1))
    live = max(1, (3 * n) // 4)
    r, c = rng.integers(0, live, m), rng.integers(0, live, m)
    keep = r != c
    diag = rng.integers(0, n, int(rng.integers(0, n // 3 + 1)))
    return rcm_cases._sym(n, r[keep], c[keep], diag)


@pytest.mark.parametrize('name', list(rcm_cases.CASES))
def test_oracle_equals_scipy_on_the_cases(name):
    rowptr, col = rcm_cases.get(name)
    seeds = ro.seed_order(rowptr, col)
    order, levels, components = ro.rcm_sorted(rowptr, col, seeds)
    assert np.array_equal(order[::-1], scipy_perm(rowptr, col))
    order2, levels2, components2 = ro.rcm_scan(rowptr, col, seeds)
    assert np.array_equal(order2, order), 'the scan form equals the sorted form'
    assert (levels2, components2) == (levels, components)
    nodes, want_levels, want_components = rcm_cases.CASES[name][1:]
    assert rowptr.size - 1 == nodes
    if want_levels is not None:
        assert (levels, components) == (want_levels, want_components)


def test_oracle_equals_scipy_on_random_graphs():
    rng = np.random.default_rng(0)
    for i in range(300):
        rowptr, col = random_graph(rng, int(rng.integers(1, 401)))
        seeds = ro.seed_order(rowptr, col)
        order, levels, components = ro.rcm_sorted(rowptr, col, seeds)
        assert np.array_equal(order[::-1], scipy_perm(rowptr, col)), i
        order2, levels2, components2 = ro.rcm_scan(rowptr, col, seeds)
        assert np.array_equal(order2, order) and (levels2, components2) == (levels, components), i
        assert np.array_equal(np.sort(order), np.arange(rowptr.size - 1))


def test_degree_counts_the_diagonal_twice():
    rowptr, col = rcm_cases.get('two_hubs')
    deg = ro.degrees(rowptr, col)
    row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    on_diag = np.zeros(rowptr.size - 1, bool)
    on_diag[row[row == col]] = True
    assert int(on_diag.sum()) == 498
    assert np.array_equal(deg, np.diff(rowptr) + on_diag)


def test_a_stable_seed_order_does_not_reproduce_scipy():
    """Rule 2 of docs/design/rcm.md: scipy seeds the components in the order of numpy's DEFAULT argsort, which is not
    stable.  If this test fails because the orders agree on every case, numpy's default sort has become stable on this
    build and the host step of seeds='scipy' could go -- until then it cannot."""
    differs = []
    for name in rcm_cases.CASES:
        rowptr, col = rcm_cases.get(name)
        if rowptr.size - 1 < 2:
            continue
        order, _, _ = ro.rcm_sorted(rowptr, col, ro.stable_seed_order(rowptr, col))
        if not np.array_equal(order[::-1], scipy_perm(rowptr, col)):
            differs.append(name)
    assert differs
