"""tests/spmm_forward_reference.py held to its own claims, without a GPU: the oracle against dense fp64 torch and the C
oracle, the vectorised and linear forms against the loops, the numpy partition against the kernel's search written out,
every builder's census against the keys it promises, the piece-wise restatement against the oracle -- and every planted
defect rejected by name."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as oc
from pytorch_sparse_amd import _native as nat
from tests import spmm_forward_reference as R

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16


def small_csr(M, N, E, seed, empties=True):
    rng = np.random.default_rng(seed)
    row = np.sort(rng.integers(0, M, E))
    if empties:
        row[row == M // 2] = M // 2 + 1 if M // 2 + 1 < M else 0
        row = np.sort(row)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=M))]).astype(np.int64)
    return rowptr, rng.integers(0, N, E).astype(np.int64)


def special_values(v, x, seed):
    """NaN, infinities and signed zeros among the operands (min / max)."""
    rng = np.random.default_rng(seed)
    x = x.copy()
    flat = x.reshape(-1)
    n = flat.size
    flat[rng.integers(0, n, n // 10)] = np.nan
    flat[rng.integers(0, n, n // 20)] = np.inf
    flat[rng.integers(0, n, n // 20)] = -np.inf
    flat[rng.integers(0, n, n // 10)] = 0.0
    flat[rng.integers(0, n, n // 10)] = -0.0
    return v, x


# ---- oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_value', [False, True])
def test_oracle_against_dense_torch(with_value):
    M, N, K, E = 23, 17, 5, 300
    rowptr, col = small_csr(M, N, E, 1)
    v, x = R.exact_operands(N, K, E, F32, 2)
    v = v if with_value else None
    row = np.repeat(np.arange(M), np.diff(rowptr))
    A = torch.zeros(M, N, dtype=torch.float64)
    A.index_put_((torch.from_numpy(row), torch.from_numpy(col)), torch.from_numpy(v if with_value else np.ones(E)),
                 accumulate=True)
    got, l1, _ = R.oracle_loops(rowptr, col, v, x, 'sum')
    assert np.array_equal(got, (A @ torch.from_numpy(x)).numpy())
    mean, _, _ = R.oracle_loops(rowptr, col, v, x, 'mean')
    assert np.array_equal(mean, got / np.maximum(np.diff(rowptr), 1)[:, None])
    assert np.all(l1 >= np.abs(got)) and np.all(got[np.diff(rowptr) == 0] == 0)
    for reduce in ('min', 'max'):
        got, _, arg = R.oracle_loops(rowptr, col, v, x, reduce, F32)
        for r in range(M):
            s, e = rowptr[r], rowptr[r + 1]
            if s == e:
                assert np.all(got[r] == 0) and np.all(arg[r] == E)
                continue
            p = torch.from_numpy(x[col[s:e]] * (v[s:e, None] if with_value else 1.0))
            want = torch.amin(p, 0) if reduce == 'min' else torch.amax(p, 0)
            assert np.array_equal(got[r], want.numpy())
            first = np.argmax(p.numpy() == want.numpy()[None], axis=0)  # numpy: the first occurrence
            assert np.array_equal(arg[r], s + first)


@pytest.mark.parametrize('reduce', ['sum', 'min', 'max'])
def test_oracle_against_c_oracle_integers(reduce):
    M, N, K, E = 40, 30, 7, 500
    rowptr, col = small_csr(M, N, E, 3)
    v, x = R.exact_operands(N, K, E, F32, 4)
    eo, ea = oc.spmm(oc.I32, reduce, rowptr, col, v.astype(np.int32), x.astype(np.int32))
    got, _, arg = R.oracle(rowptr, col, v, x, reduce, F32)
    filled = np.diff(rowptr) > 0
    assert np.array_equal(got[filled], eo[filled].astype(np.float64))
    if ea is not None:
        assert np.array_equal(arg, ea)
    fo, fa = oc.spmm(oc.F32, reduce, rowptr, col, v.astype(np.float32), x.astype(np.float32))
    assert np.array_equal(got.astype(np.float32), fo) and (fa is None or np.array_equal(arg, fa))


@pytest.mark.parametrize('dtype', [F32, BF16, F64])
@pytest.mark.parametrize('reduce', R.REDUCES)
def test_vectorised_oracle_equals_loops(dtype, reduce):
    M, N, K, E = 37, 19, 6, 900
    rowptr, col = small_csr(M, N, E, 5)
    v, x = R.real_operands(N, K, E, dtype, 6, B=2)
    if reduce in ('min', 'max'):
        v, x = special_values(v, x, 7)
    a = R.oracle_loops(rowptr, col, v, x, reduce, dtype)
    for chunk in (1 << 23, 64):  # one block of rows, and many
        b = R.oracle(rowptr, col, v, x, reduce, dtype, chunk=chunk)
        if reduce in ('min', 'max'):
            assert np.array_equal(R.bits_of(torch.from_numpy(a[0])), R.bits_of(torch.from_numpy(b[0])))
            assert np.array_equal(a[2], b[2])
        else:  # two summation orders of the same terms
            tol = 4 * float(np.finfo(a[0].dtype).eps) * np.diff(rowptr).max() * b[1]
            assert np.all(np.abs(a[0] - b[0]) <= tol) and np.all(np.abs(a[1] - b[1]) <= tol)
    v, x = R.exact_operands(N, K, E, dtype, 8, B=2)  # small integers: the two forms agree exactly
    a, b = R.oracle_loops(rowptr, col, v, x, reduce, dtype), R.oracle(rowptr, col, v, x, reduce, dtype, chunk=64)
    assert np.array_equal(a[0], b[0]) and (a[2] is None or np.array_equal(a[2], b[2]))


def test_row_without_a_winner_and_signed_zeros():
    rowptr = np.array([0, 3, 3, 6, 8], np.int64)
    col = np.array([0, 0, 0, 1, 2, 1, 3, 3], np.int64)
    x = np.array([[np.nan, -R.INIT[F32]], [-0.0, 1.0], [0.0, 1.0], [-np.inf, np.nan]])
    for f in (R.oracle_loops, R.oracle):
        out, _, arg = f(rowptr, col, None, x, 'max', F32)
        assert np.array_equal(arg, [[8, 8], [8, 8], [3, 3], [8, 8]])  # NaN, the init value itself and -inf never win
        assert out[0, 0] == -R.INIT[F32] and np.all(out[1] == 0) and np.signbit(out[2, 0]) and out[3, 1] == -R.INIT[F32]


def test_linear_oracles_against_loops():
    M, N, K, E = 50, 8, 9, 2000
    rowptr, col = small_csr(M, N, E, 9)
    v, x = R.exact_operands(N, K, E, F32, 10)
    for reduce in ('sum', 'mean'):
        a, b = R.oracle_loops(rowptr, col, v, x, reduce), R.linear_oracle(rowptr, col, v, x, reduce, N)
        assert np.allclose(a[0], b[0], rtol=1e-14, atol=0) and np.allclose(a[1], b[1], rtol=1e-14, atol=0)
        if reduce == 'sum':
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    x[2, 3] = x[5, 3] = 8.0  # two columns tie in one feature: the first entry of either wins
    x[1, 0] = np.nan
    for reduce in ('min', 'max'):
        a, b = R.oracle_loops(rowptr, col, None, x, reduce, F32), R.linear_minmax(rowptr, col, x, reduce, N, F32, 16)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[1])


# ---- partition --------------------------------------------------------------------------------------------------
def kernel_search(rowptr, items, snap):
    """spmm_partition_kernel, line by line"""
    M, E = len(rowptr) - 1, int(rowptr[-1])
    P = -(-max(M + E, 1) // items)
    out = []
    for p in range(P + 1):
        d = min(p * items, M + E)
        lo, hi = max(d - E, 0), min(d, M)
        while lo < hi:
            mid = (lo + hi) >> 1
            if rowptr[mid + 1] <= d - mid - 1:
                lo = mid + 1
            else:
                hi = mid
        e = d - lo
        if snap > 0 and lo < M:
            rs = rowptr[lo]
            if e > rs and e - rs <= snap:
                e = rs
        out.append((lo, e))
    return np.array(out, np.int64)


@pytest.mark.parametrize('snap', [0, 64])
def test_numpy_partition_is_the_kernels_search(snap):
    graphs = [R.build_chains(128)[0], R.build_ties(128, 64)[0], R.build_short(128, 4)[0], R.build_skewed(1024)[0],
              np.array([0, 0, 0, 0], np.int64), np.array([0, 700], np.int64), np.zeros(300, np.int64)]
    for rowptr in graphs:
        for items in (128, 200):
            t = R.partition(rowptr, items, snap)
            assert np.array_equal(t, kernel_search(rowptr, items, snap))
            assert np.all(np.diff(t[:, 0]) >= 0) and np.all(np.diff(t[:, 1]) >= 0), 'the table is monotonic'


# ---- builders ---------------------------------------------------------------------------------------------------
def route_of(rowptr, dtype, reduce, N, K, B=1):
    return nat.spmm_route(dtype, reduce, B, len(rowptr) - 1, N, K, int(rowptr[-1]))


def test_chain_builder_reaches_every_fixup_branch():
    rowptr, keys = R.build_chains(128)
    r = route_of(rowptr, F32, 'sum', 64, 64)
    assert r['items'] == 128 and r['fixup'] == 1
    c = R.census(rowptr, R.partition(rowptr, r['items']), r['items'])
    for run in keys['run_hist']:
        assert c['run_hist'].get(run, 0) >= 1, 'no cut row with %d tail records' % run
    assert {1, 2, 7, 8, 9, 16, 63, 64, 65, 128, 199} <= set(c['run_hist'])
    for k in ('empty_head', 'cut_last_row', 'inside_one_row', 'boundary_on_row_start', 'incoming_row_ends'):
        assert c[k] >= keys[k], k
    deg = np.diff(rowptr)
    one_in = [R_ for R_, run in c['runs'].items() if deg[R_] == 40]
    assert one_in and c['runs'][one_in[0]] == 1
    assert R.exact_operands_ok(rowptr, F32) and R.exact_operands_ok(rowptr, F16)
    # with the min / max snap the same rows are cut into the same chains (only short rows move)
    rm = route_of(rowptr, F32, 'max', 64, 64)
    cm = R.census(rowptr, R.partition(rowptr, rm['items'], rm['snap']), rm['items'], rm['snap'])
    assert {1, 2, 7, 8, 9, 16, 63, 64, 65, 128, 199} <= set(cm['run_hist']) and cm['snapped'] >= 1


def test_small_builders():
    rowptr, keys = R.build_one_row(128)
    c = R.census(rowptr, R.partition(rowptr, 128), 128)
    assert c['run_hist'] == {3: 1} and c['cut_last_row'] == 1 and c['P'] == 4
    for P in (1, 2):
        rowptr, _ = R.build_partitions(128, P)
        assert route_of(rowptr, F32, 'sum', 64, 64)['P'] == P
        assert route_of(rowptr, F32, 'sum', 64, 64)['fixup'] == P - 1
    rowptr, _ = R.build_skewed(1024)
    for K, dtype in ((64, F32), (65, F32), (66, BF16), (8, F64)):
        r = route_of(rowptr, dtype, 'sum', 500, K)
        c = R.census(rowptr, R.partition(rowptr, r['items']), r['items'])
        assert c['cut_rows'] >= 10 and c['P'] > 8 and max(c['run_hist']) >= 3


def test_ties_builder():
    r = route_of(R.build_ties(128, 64)[0], F32, 'max', 64, 64)
    assert (r['items'], r['snap']) == (128, 64)
    rowptr, keys, named = R.build_ties(r['items'], r['snap'])
    c = R.census(rowptr, R.partition(rowptr, r['items'], r['snap']), r['items'], r['snap'])
    assert c['runs'][named['long']] == 69
    assert named['nan'] in c['runs'] and named['zeros'] in c['runs']
    assert named['snap'] not in c['runs'], 'a row of `snap` entries is never cut'
    assert c['runs'].get(named['snap1']) == 1, 'a row of snap + 1 entries is'
    assert c['snapped'] >= 1
    c0 = R.census(rowptr, R.partition(rowptr, r['items'], 0), r['items'], 0)
    assert named['snap'] in c0['runs'], 'without the snap that row straddles a boundary'


@pytest.mark.parametrize('K,dtype', [(4, F32), (8, F32), (16, F32), (32, F32), (8, BF16), (32, BF16), (16, F64)])
def test_short_builder_reaches_every_batching_decision(K, dtype):
    probe = nat.spmm_route(dtype, 'sum', 1, 1000, 64, K, 5000)
    assert probe['family'] == 'short'
    rowptr, keys = R.build_short(probe['items'], probe['lgG'])
    r = route_of(rowptr, dtype, 'sum', 64, K)
    assert (r['items'], r['lgG'], r['family']) == (probe['items'], probe['lgG'], 'short')
    c = R.short_census(rowptr, R.partition(rowptr, r['items']), r['lgG'])
    for k in keys:
        assert c[k] >= 1, (k, c)
    G = 1 << r['lgG']
    assert c['longest_batch'] == G and {2, G} <= set(c['batch_sizes'])


@pytest.mark.parametrize('dtype,K,total,items', R.LENGTH_CASES)
def test_partition_length_builder(dtype, K, total, items):
    rowptr = R.build_total(4096, total)
    assert len(rowptr) == 4097 and 4096 + int(rowptr[-1]) == total and R.exact_operands_ok(rowptr, dtype)
    for reduce, snap in (('sum', 0), ('max', min(128, items // 2))):
        r = route_of(rowptr, dtype, reduce, 64, K)
        assert (r['items'], r['snap'], r['P']) == (items, snap, -(-total // items))
        c = R.census(rowptr, R.partition(rowptr, items, snap), items, snap)
        assert c['cut_rows'] >= 100 and max(c['run_hist']) >= 64 and c['inside_one_row'] >= 64
        assert snap == 0 or c['snapped'] >= 1
    assert items in (256, 512, 1024) or items % 64 != 0


# ---- the piece-wise restatement and the planted defects -------------------------------------------------------------
def graph_for(defect):
    """(rowptr, N, K, B, reduce) on which the defect shows"""
    if defect in ('tie_to_larger_id', 'tail_widened_with_wrong_partition'):
        return R.build_ties(128, 64)[0], 16, 8, None, 'max'
    if defect == 'last_packet_skipped':
        return R.build_skewed(256, seed=1)[0], 40, 66, None, 'sum'
    if defect == 'batch1_reads_batch0':
        return R.build_skewed(256, seed=2)[0], 40, 8, 2, 'sum'
    if defect == 'limit_row_loses_last_entry':
        return R.build_short(128, 5)[0], 40, 8, None, 'sum'
    return R.build_chains(128)[0], 40, 8, None, 'mean' if defect == 'mean_by_piece_length' else 'sum'


def run_pieces(rowptr, N, K, B, reduce, dtype, operands, defect=None, seed=11):
    E = int(rowptr[-1])
    col = R.columns(E, N, seed)
    v, x = operands(N, K, E, dtype, seed + 1, B=B)
    if reduce in ('min', 'max') and operands is R.exact_operands:
        v = None
        x = np.minimum(np.abs(x), 2.0)  # many equal candidates: ties in every piece and across pieces
    r = nat.spmm_route(dtype, reduce, 1 if B is None else B, len(rowptr) - 1, N, K, E)
    table = R.partition(rowptr, r['items'], r['snap'])
    got, arg = R.piecewise(rowptr, col, v, x, reduce, dtype, r, table, defect)
    return got, arg, R.oracle(rowptr, col, v, x, reduce, dtype)


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('reduce', R.REDUCES)
def test_restatement_equals_the_oracle(dtype, reduce):
    for rowptr, N, K, B in [(R.build_chains(128)[0], 40, 8, None), (R.build_ties(128, 64)[0], 16, 8, None),
                            (R.build_short(128, 5)[0], 40, 8, 2), (R.build_skewed(256, seed=1)[0], 40, 66, None),
                            (R.build_one_row(128)[0], 40, 12, None), (R.build_partitions(128, 1)[0], 40, 8, None),
                            (R.build_partitions(128, 2)[0], 40, 8, 2), (R.build_total(64, 20000), 40, 8, None)]:
        assert R.exact_operands_ok(rowptr, dtype)
        got, arg, (exact, l1, want_arg) = run_pieces(rowptr, N, K, B, reduce, dtype, R.exact_operands)
        if reduce in ('min', 'max'):
            assert R.minmax_mismatches(got, torch.from_numpy(arg), exact, want_arg, dtype) == 0
            continue
        if reduce == 'sum':
            assert R.exact_mismatches(got, exact, dtype) == 0
        assert R.real_violations(got, exact, l1, rowptr, dtype, reduce)[0] == 0
        # real values: float32 numpy sums of every piece stay inside the derived bound
        got, _, (exact, l1, _) = run_pieces(rowptr, N, K, B, reduce, dtype, R.real_operands)
        bad, worst = R.real_violations(got, exact, l1, rowptr, dtype, reduce)
        assert bad == 0, worst


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_planted_defect_is_rejected(defect):
    rowptr, N, K, B, reduce = graph_for(defect)
    got, arg, (exact, l1, want_arg) = run_pieces(rowptr, N, K, B, reduce, F32, R.exact_operands, defect)
    if reduce in ('min', 'max'):
        assert R.minmax_mismatches(got, torch.from_numpy(arg), exact, want_arg, F32) > 0
        return
    if reduce == 'sum':
        assert R.exact_mismatches(got, exact, F32) > 0, 'the exact comparator lets %s pass' % defect
    assert R.real_violations(got, exact, l1, rowptr, F32, reduce)[0] > 0
    # none of these defects is below rounding: real values catch them too, at both element types
    for dtype in (F32, BF16):
        got, _, (exact, l1, _) = run_pieces(rowptr, N, K, B, reduce, dtype, R.real_operands, defect)
        assert R.real_violations(got, exact, l1, rowptr, dtype, reduce)[0] > 0, dtype


def test_bound_is_never_looser_than_the_projects():
    rowptr = np.array([0, 1, 11, 10011], np.int64)
    l1 = np.ones((3, 2))
    for dtype in R.FLOATS:
        b = R.real_bound(l1 * 0.5, l1, rowptr, dtype, 'sum')
        assert np.all(b <= R.SUM_TOL[dtype] * l1 + R.SUM_ATOL[dtype])
    assert R.real_bound(l1 * 0.5, l1, rowptr, F32, 'sum')[0, 0] == 3 * 2.0 ** -24  # one product: (1 + 2) u, no u_out
    assert R.real_bound(l1 * 0.5, l1, rowptr, BF16, 'sum')[0, 0] == 3 * 2.0 ** -24 + 2.0 ** -9
    assert R.real_bound(l1 * 0.5, l1, rowptr, BF16, 'sum')[0, 0] < 0.3 * R.SUM_TOL[BF16]
