"""Reverse Cuthill-McKee on the GPU (csrc/rcm.hip, csrc/ops_rcm.cpp, docs/design/rcm.md): tsamd::rcm against the numpy
oracle of tests/rcm_oracle.py -- itself checked against scipy in tests/test_rcm_oracle.py -- at capacities that push the
levels across the two routes in both directions, the bound on host round trips, and the public call against scipy with
scipy's ordering made unavailable.  Every comparison is exact."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pytorch_sparse_amd as ts
from tests import rcm_cases, rcm_oracle as ro

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OPS = torch.ops.tsamd
STATS = ('levels', 'components', 'big_levels', 'small_launches', 'host_syncs')


def dev(x):
    return torch.from_numpy(np.asarray(x, np.int64).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(seed order, perm, levels, components) of a case by the oracle, computed once and shared."""
    rowptr, col = rcm_cases.get(name)
    seeds = ro.seed_order(rowptr, col)
    perm, levels, components = ro.rcm(rowptr, col, seeds)
    for a in (seeds, perm):
        a.setflags(write=False)
    return seeds, perm, levels, components


def run(name, small_cap):
    rowptr, col = rcm_cases.get(name)
    seeds = expected(name)[0]
    perm, stats = OPS.rcm(dev(rowptr), dev(col), dev(seeds), small_cap)
    assert perm.dtype == torch.int64 and stats.dtype == torch.int64
    return perm.cpu().numpy(), dict(zip(STATS, stats.tolist()))


def caps():
    return (-1, 0, int(OPS.rcm_limits()[0]), 64)


@pytest.mark.parametrize('name', list(rcm_cases.CASES))
def test_rcm_equals_the_oracle_at_every_capacity(name):
    _, want, levels, components = expected(name)
    for cap in caps():
        perm, stats = run(name, cap)
        assert np.array_equal(perm, want), (name, cap)
        assert (stats['levels'], stats['components']) == (levels, components), (name, cap, stats)
        if cap == 0:  # every level runs on the whole device, bar the isolated nodes the seed search emits itself
            rowptr = rcm_cases.get(name)[0]
            assert stats['big_levels'] == levels - int((np.diff(rowptr) == 0).sum()), (name, stats)


def test_both_routes_run():
    """The shipped capacity really alternates: the star's hub level and the skewed graph's wide levels leave the one
    workgroup, the levels after them return to it."""
    for name in ('star', 'skewed', 'uniform'):
        _, stats = run(name, -1)
        assert 0 < stats['big_levels'] < stats['levels'], (name, stats)
    _, stats = run('grid', 64)
    assert stats['big_levels'] == 0, 'the grid never has more than 40 nodes in a frontier'
    _, stats = run('many_components', 64)
    assert 0 < stats['big_levels'] < stats['levels']


@pytest.mark.parametrize('name', list(rcm_cases.CASES))
def test_host_round_trips_are_bounded(name):
    budget = int(OPS.rcm_limits()[2])
    _, stats = run(name, -1)
    bound = 4 + 2 * stats['big_levels'] + 2 * math.ceil(stats['levels'] / budget)
    assert stats['host_syncs'] <= bound, (stats, bound)
    if name in ('path', 'many_components'):
        assert stats['big_levels'] == 0


def test_limits():
    nodes, entries, budget = OPS.rcm_limits()
    assert nodes >= 64 and entries >= nodes and budget >= 1


def test_rcm_degree_counts_the_diagonal():
    rowptr, col = rcm_cases.get('two_hubs')
    deg = OPS.rcm_degree(dev(rowptr), dev(col))
    assert deg.dtype == torch.int64
    assert np.array_equal(deg.cpu().numpy(), ro.degrees(rowptr, col))


def test_rcm_refuses_seeds_that_are_no_permutation():
    rowptr, col = rcm_cases.get('grid')
    seeds = expected('grid')[0].copy()
    seeds[5] = seeds[6]
    with pytest.raises(RuntimeError, match='permutation'):
        OPS.rcm(dev(rowptr), dev(col), dev(seeds), -1)
    seeds[5] = rowptr.size + 3
    with pytest.raises(RuntimeError, match='permutation'):
        OPS.rcm(dev(rowptr), dev(col), dev(seeds), -1)


@pytest.mark.parametrize('small_cap', [-1, 0])
def test_rcm_refuses_a_repeated_isolated_seed(small_cap):
    """Isolated seeds are written out in batches by the seed search; a repeated one would take two positions there and
    push the search past the end of `order`.  The flag tsamd_rcm_begin raises stops the first launch before it runs.  The
    seeds here are repeated isolated pairs in front of the blob's seeds, the shape that overruns the furthest."""
    rowptr, col = rcm_cases.get('many_components')
    seeds = expected('many_components')[0].copy()
    isolated = np.diff(rowptr)[seeds] == 0
    first = np.nonzero(isolated)[0]
    assert first.size == 700
    seeds[first[1::2]] = seeds[first[0::2]]
    with pytest.raises(RuntimeError, match='permutation'):
        OPS.rcm(dev(rowptr), dev(col), dev(seeds), small_cap)
    # the device is intact and the op still answers
    perm, _ = run('many_components', small_cap)
    assert np.array_equal(perm, expected('many_components')[1])


# ---- the public call ----------------------------------------------------------------------------------------------------
def unsymmetric():
    """1500 nodes, 6000 directed entries with float values, a few diagonals: to_symmetric has work to do."""
    rng = np.random.default_rng(7)
    key = np.unique(rng.integers(0, 1500 * 1500, 6000))
    key = np.union1d(key, np.arange(0, 1500, 50) * 1501)
    val = rng.integers(1, 100, key.size).astype(np.float32)
    return sp.csr_matrix((val, (key // 1500, key % 1500)), shape=(1500, 1500))


def case_matrix(name):
    rowptr, col = rcm_cases.get(name)
    n = rowptr.size - 1
    val = np.random.default_rng(8).integers(1, 100, col.size).astype(np.float32)
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


def to_sparse_tensor(S):
    coo = S.tocoo()
    return ts.SparseTensor(row=dev(coo.row), col=dev(coo.col), value=torch.from_numpy(coo.data).to(DEV),
                           sparse_sizes=S.shape)


@pytest.mark.parametrize('which', ['uniform', 'many_components', 'unsymmetric'])
def test_public_call_equals_scipy_without_calling_it(which, monkeypatch):
    S = unsymmetric() if which == 'unsymmetric' else case_matrix(which)
    A = to_sparse_tensor(S)
    sym = (S + S.T).tocsr()
    want_perm = sp.csgraph.reverse_cuthill_mckee(sym, symmetric_mode=True).astype(np.int64)
    want = sym[want_perm][:, want_perm].tocsr()
    want.sort_indices()

    def refuse(*args, **kwargs):
        raise AssertionError('the GPU path must not call scipy for the ordering')
    monkeypatch.setattr(sp.csgraph, 'reverse_cuthill_mckee', refuse)
    out, perm = ts.reverse_cuthill_mckee(A)
    assert np.array_equal(perm.cpu().numpy(), want_perm)
    rowptr, col, value = out.csr()
    assert np.array_equal(rowptr.cpu().numpy(), want.indptr.astype(np.int64))
    assert np.array_equal(col.cpu().numpy(), want.indices.astype(np.int64))
    assert np.array_equal(value.cpu().numpy(), want.data)
    out2, perm2 = A.reverse_cuthill_mckee()
    assert torch.equal(perm2, perm), 'two calls are bit-identical'
    assert all(torch.equal(a, b) for a, b in zip(out2.csr(), out.csr()))


def test_stable_seeds_equal_the_oracle_seeded_stably():
    for name in ('many_components', 'two_hubs'):
        rowptr, col = rcm_cases.get(name)
        A = to_sparse_tensor(case_matrix(name))
        _, perm = ts.reverse_cuthill_mckee(A, True, seeds='stable')
        deg = ro.degrees(rowptr, col)
        want, _, _ = ro.rcm(rowptr, col, np.argsort(deg, kind='stable'))
        assert np.array_equal(perm.cpu().numpy(), want), name
        _, again = ts.reverse_cuthill_mckee(A, True, seeds='stable')
        assert torch.equal(again, perm)
