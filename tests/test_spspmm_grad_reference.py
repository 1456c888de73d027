"""The reference of the SpSpMM value gradients (tests/spspmm_grad_reference.py) is itself held to account before the
GPU is asked anything: its oracle equals dense autograd and torch.sparse.mm's autograd, every builder reaches what it
was built for (census, from the route words of tsamd_spspmm_bw_route), and the comparator that the GPU test uses
rejects six planted defects.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import spspmm_grad_reference as R
from tests import util

F32, F64 = 0, 1


def route_words():
    w32, w64 = nat.spspmm_bw_route(torch.float32), nat.spspmm_bw_route(torch.float64)
    assert w32 == w64
    return w32


def lg_range(dtype):
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spspmm_route(F32 if dtype == 'f32' else F64, ctypes.c_int64(2 ** 32 - 2), out) == 0
    return int(out[0])


def setup():
    w = route_words()
    return w[0], w[1]


def test_route_words_and_refusals():
    w = route_words()
    assert w[0] >= 64 and w[0] % 64 == 0 and w[0] <= R.MAX_TILE  # products per tile
    assert w[1] >= 1                                             # segments a tile may stage
    assert w[0] % w[2] == 0 and w[3] == 2 and w[4:] == [0, 0, 0, 0]
    out = (ctypes.c_int64 * 8)()
    L = nat.lib()
    assert L.tsamd_spspmm_bw_route(2, out) == 2      # fp16
    assert L.tsamd_spspmm_bw_route(5, out) == 2      # int64
    assert L.tsamd_spspmm_bw_route(F32, None) == 1
    assert L.tsamd_spspmm_bw_workspace_bytes(F32, ctypes.c_int64(0)) > 0
    # two records per tile, nothing proportional to the products beyond that: 2.29 G products -> tens of MB
    assert L.tsamd_spspmm_bw_workspace_bytes(F64, ctypes.c_int64(2_290_000_000)) < 64 * 2_290_000_000 // w[0]


def test_bounds_are_the_projects():
    assert R.SUM_TOL == {'f32': util.SUM_TOL[torch.float32], 'f64': util.SUM_TOL[torch.float64]}
    assert R.SUM_ATOL == {'f32': util.SUM_ATOL[torch.float32], 'f64': util.SUM_ATOL[torch.float64]}


def _random_pair(seed, m=40, k=30, n=50, density=0.15):
    rng = np.random.default_rng(seed)
    a = [np.nonzero(rng.random(k) < density)[0] for _ in range(m)]
    b = [np.nonzero(rng.random(n) < density)[0] for _ in range(k)]
    a[3], b[5] = [], []
    return R.make_pair('random%d' % seed, a, b, n)


@pytest.mark.parametrize('mode', ['both', 'a_only', 'b_only'])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_oracle_equals_dense_autograd(seed, mode):
    case = _random_pair(seed)
    va, vb, g = R.values(case, 'uniform', seed)
    m, k, n = case['m'], case['k'], case['N']
    ta = torch.tensor(va if mode != 'b_only' else np.ones_like(va), requires_grad=True)
    tb = torch.tensor(vb if mode != 'a_only' else np.ones_like(vb), requires_grad=True)
    A = torch.zeros(m, k, dtype=torch.float64).index_put((torch.from_numpy(case['rowA']), torch.from_numpy(case['colA'])), ta)
    B = torch.zeros(k, n, dtype=torch.float64).index_put((torch.from_numpy(case['rowB']), torch.from_numpy(case['colB'])), tb)
    C = A @ B
    vc = C[torch.from_numpy(case['rowC']), torch.from_numpy(case['colC'])]
    vc.backward(torch.from_numpy(g))
    gA, gB, l1A, l1B = R.oracle(case, va if mode != 'b_only' else None, vb if mode != 'a_only' else None, g)
    assert np.abs(gA - ta.grad.numpy()).max() <= 1e-13 * max(1.0, l1A.max())
    assert np.abs(gB - tb.grad.numpy()).max() <= 1e-13 * max(1.0, l1B.max())
    assert l1A.min() >= 0 and bool((np.abs(gA) <= l1A + 1e-300).all()) and bool((np.abs(gB) <= l1B + 1e-300).all())
    # the pattern of C is the structural one: every product has its entry
    assert case['prodC'].size == case['prodA'].size and int(case['prodC'].max()) == case['colC'].size - 1


@pytest.mark.parametrize('seed', [0, 1])
def test_oracle_equals_torch_sparse_mm_autograd(seed):
    """The contract of the issue: torch.sparse.mm is differentiable in both value tensors, and its gradients are the
    dense formula restricted to the operands' patterns.  Positive values, so that no entry of the product cancels and
    the two patterns coincide (asserted)."""
    case = _random_pair(10 + seed)
    rng = np.random.default_rng(seed)
    va, vb = rng.random(case['colA'].size) + 0.5, rng.random(case['colB'].size) + 0.5
    g = rng.random(case['colC'].size) - 0.5
    ta, tb = torch.tensor(va, requires_grad=True), torch.tensor(vb, requires_grad=True)
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([case['rowA'], case['colA']])), ta, (case['m'], case['k']))
    B = torch.sparse_coo_tensor(torch.from_numpy(np.stack([case['rowB'], case['colB']])), tb, (case['k'], case['N']))
    C = torch.sparse.mm(A, B).coalesce()
    idx = C.indices().numpy()
    assert np.array_equal(idx[0], case['rowC']) and np.array_equal(idx[1], case['colC'])
    C.values().backward(torch.from_numpy(g))
    gA, gB, l1A, l1B = R.oracle(case, va, vb, g)
    assert ta.grad is not None and tb.grad is not None
    assert np.abs(gA - ta.grad.numpy()).max() <= 1e-13 * max(1.0, l1A.max())
    assert np.abs(gB - tb.grad.numpy()).max() <= 1e-13 * max(1.0, l1B.max())


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_census_of_every_builder(dtype):
    T, limit = setup()
    cases = R.builders(T, limit, lg_range(dtype))
    assert set(cases) == {'long_row', 'tall_col', 'aligned', 'empties', 'wide', 'unstaged'}
    R.assert_census(cases, T, limit)
    for c in cases.values():  # sorted rows, unique entries: the operands the contract names
        for ptr, col in ((c['rowptrA'], c['colA']), (c['rowptrB'], c['colB']), (c['rowptrC'], c['colC'])):
            inner = np.ones(col.size, bool)
            inner[ptr[1:-1][ptr[1:-1] < col.size]] = False
            assert bool((np.diff(col)[inner[1:]] > 0).all())


def test_builders_refuse_a_larger_tile():
    with pytest.raises(AssertionError):
        R.long_row(R.MAX_TILE + 64)
    with pytest.raises(AssertionError):
        R.unstaged(2 * R.MAX_TILE, 2048)


def _list_values(side, va, vb):
    return vb if side == 0 else va


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['dyadic', 'uniform'])
def test_restated_kernel_passes_the_checker(dtype, kind):
    T, limit = setup()
    lg = lg_range(dtype)
    for name, case in R.builders(T, limit, lg).items():
        for mode in ('both', 'a_only', 'b_only'):
            va, vb, g, gA, gB, l1A, l1B = R.expected(T, limit, lg, name, kind, dtype, mode)
            R.check_grad(R.emulate(case, 0, vb, g, dtype, T), gA, l1A, dtype, kind, '%s gA %s' % (name, mode))
            R.check_grad(R.emulate(case, 1, va, g, dtype, T), gB, l1B, dtype, kind, '%s gB %s' % (name, mode))


# defect -> (builder, side, mode) on which the comparator has to reject it
PLANTED = {
    'last_term_dropped': ('long_row', 0, 'both'),
    'lookup_off_by_one': ('aligned', 0, 'both'),
    'row_order_on_column_side': ('tall_col', 1, 'both'),
    'empty_unwritten': ('empties', 0, 'both'),
    'missing_value_is_zero': ('long_row', 0, 'a_only'),
    'carry_twice': ('tall_col', 1, 'both'),
}


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['dyadic', 'uniform'])
@pytest.mark.parametrize('defect', R.DEFECTS)
def test_planted_defects_are_rejected(defect, kind, dtype):
    assert set(PLANTED) == set(R.DEFECTS) and len(R.DEFECTS) >= 6
    T, limit = setup()
    lg = lg_range(dtype)
    name, side, mode = PLANTED[defect]
    case = R.builders(T, limit, lg)[name]
    va, vb, g, gA, gB, l1A, l1B = R.expected(T, limit, lg, name, kind, dtype, mode)
    exact, l1 = (gA, l1A) if side == 0 else (gB, l1B)
    w = _list_values(side, va, vb)
    R.check_grad(R.emulate(case, side, w, g, dtype, T), exact, l1, dtype, kind)  # the clean restatement passes
    bad = R.emulate(case, side, w, g, dtype, T, defect=defect)
    with pytest.raises(AssertionError):
        R.check_grad(bad, exact, l1, dtype, kind)
