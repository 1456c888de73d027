"""The numpy oracle of the partitioner (tests/partition_oracle.py) held to what docs/design/partition.md promises, on
the inputs of tests/test_partition_gpu.py, without a GPU -- an oracle nobody validated would only be a second copy of
the bugs -- and the branch counters of every case family that tests/test_partition_exact_gpu.py compares on the
device, so that those comparisons cannot pass without reaching the branch they are named for."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import partition_cases as pc
from tests import partition_oracle as po
from tests import partition_reference as pr
from tests.test_partition_gpu import QUALITY


def counted(f, *args):
    po.reset_counters()
    out = f(*args)
    return out, dict(po.COUNTERS)


# ---- the pieces ---------------------------------------------------------------------------------------------------------
def test_tie_hash_is_a_32_bit_mix():
    ids = np.concatenate([np.arange(300), [(1 << 31) - 1, 123456789]])
    for rnd in (0, 1, 3):
        want = np.array([po.tie_hash(rnd, int(i)) for i in ids])
        assert want.max() <= po.MASK and np.array_equal(po.tie_hash_array(rnd, ids), want)
    assert len({po.tie_hash(0, i) for i in range(4096)}) == 4096, 'an invertible mix: no two ids collide'
    assert po.tie_hash(0, 0) == 0 and po.tie_hash(1, 0) != po.tie_hash(2, 0)
    # the three steps written out for one value
    x = (2 * 0x9E3779B1 + 77 * 0x85EBCA77) % (1 << 32)
    x ^= x >> 15
    x = x * 0x2C1B3C6D % (1 << 32)
    x ^= x >> 12
    x = x * 0x297A2D39 % (1 << 32)
    assert po.tie_hash(2, 77) == x ^ (x >> 15)


def check_matching(A, vw, cap, match, cmap, n_c):
    n = A.shape[0]
    D = sp.csr_matrix(A)
    for v in np.nonzero(match >= 0)[0]:
        m = match[v]
        assert m != v and D.indptr[v] != D.indptr[v + 1] and m in D.indices[D.indptr[v]:D.indptr[v + 1]]
        assert match[m] == v and vw[v] + vw[m] <= cap
    assert n_c == n - (match >= 0).sum() // 2 and np.array_equal(np.unique(cmap), np.arange(n_c))
    pair = match >= 0
    assert np.array_equal(cmap[pair], cmap[match[pair]])


@pytest.mark.parametrize('name', sorted(pc.match_cases()))
def test_match_invariants_and_counters(name):
    A, vw, cap = pc.match_cases()[name]
    states, c = counted(lambda: list(po.match_rounds(A, vw, cap, 4)))
    assert (states[0][0] < 0).all() and states[0][2] == A.shape[0]
    for before, after in zip(states, states[1:]):
        check_matching(A, vw, cap, *after)
        kept = before[0] >= 0
        assert np.array_equal(after[0][kept], before[0][kept]), 'a pair stays a pair'
    assert states[1][2] < A.shape[0], 'round 0 matches something'
    assert c['match_ties'] > 0
    if name == 'unit_grid':
        assert (A.data == 1).all(), 'all ties: the hash decides the whole matching'
    if name == 'rmat9':
        assert c['match_cap_blocked'] > 0 and c['match_rows_wave'] > 0
    if name == 'hubs':
        hubs = np.flatnonzero(np.diff(A.indptr) > 1)
        assert np.diff(A.indptr)[hubs].tolist() == [31, 32, 33, 63, 64, 65, 200]
        assert c['match_cap_blocked'] >= 7 and c['match_ties_wave'] >= 5
        for h in hubs:   # round 0: one of the five leaves of weight 50, never the heaviest (too heavy) leaf
            m = states[1][0][h]
            assert m >= 0 and A[h, m] == 50 and A[h].max() == 100


def test_match_existing_small_cases():
    A = pc.sym_from_edges(2, [0], [1])
    assert po.match(A, np.ones(2), 2, 4)[0].tolist() == [1, 0] and po.match(A, np.ones(2), 1, 4)[0].tolist() == [-1, -1]
    n = 206
    A = pc.sym_from_edges(n, np.zeros(200, np.int64), np.arange(1, 201))
    m = po.match(A, np.ones(n), 2, 4)[0]
    assert m[0] >= 1 and (m[1:201] >= 0).sum() == 1 and (m[201:] < 0).all()


def test_level0_and_contract():
    A = pr.rmat(9, 4, seed=3) + sp.eye(512, dtype=np.int64, format='csr')
    A = sp.csr_matrix(A)
    A.sort_indices()
    L = po.level0(A.indptr, A.indices)
    want = (A + A.T).tocsr()
    want.setdiag(0)
    want.eliminate_zeros()
    assert (L != want).nnz == 0 and L.diagonal().sum() == 0 and (L != L.T).nnz == 0
    G = pr.grid(9, 11, seed=3)[0]
    assert (po.level0(G.indptr, G.indices) != 2 * G).nnz == 0, 'a symmetric input carries every weight twice'
    rs = np.random.RandomState(2)
    vw, cmap = rs.randint(1, 5, 99), rs.permutation(99) % 40
    C, vw_c = po.contract(po.csr(G), vw, cmap, 40)
    want, want_vw = pr.contract_oracle(G, vw, cmap)
    assert (C != want).nnz == 0 and np.array_equal(vw_c, want_vw)
    Z = po.level0(np.array([0, 1, 1]), np.array([1]), np.array([0]))
    assert Z.nnz == 2 and Z.data.tolist() == [0, 0], 'a zero-weight edge stays an entry'


@pytest.mark.parametrize('name', sorted(pc.initial_cases()))
def test_initial_within_one_vertex_weight_and_counters(name):
    A, vw, k = pc.initial_cases()[name]
    part, c = counted(po.initial, A, vw, k)
    assert part.shape == (A.shape[0],) and part.min() >= 0 and part.max() < k
    pw = po.part_weights(part, vw, k)
    if vw.sum() > 0:
        assert np.abs(pw - vw.sum() / k).max() <= vw.max(), (pw, vw.sum() / k)
    want = {'five_components': ('bfs_components', 5), 'no_edges': ('bfs_isolated', 9), 'zero_weights': ('initial_zero_total', 1),
            'seed_tie': ('bfs_seed_ties', 1), 'k_above_n': ('bfs_seed_ties', 1)}
    if name in want:
        assert c.get(want[name][0], 0) == want[name][1], c
    if name == 'five_components':
        assert c['bfs_isolated'] == 3 and len(np.unique(part)) == 4
    if name == 'zero_weights':
        assert np.bincount(part, minlength=k).max() - np.bincount(part, minlength=k).min() <= 1
    if name == 'seed_tie':
        comp, level = po.bfs_keys(A)
        assert level.tolist() == [1, 2, 3, 0, 4], 'the search starts at vertex 3: minimum degree, then id'
    if name == 'k_above_n':
        assert k > A.shape[0] and pw.max() == 1


def test_conn_graph_reaches_every_route_and_rule():
    A, vw, part, blocked = pc.conn_graph()
    k = pc.CONN_K
    pw = po.part_weights(part, vw, k)
    deg = np.diff(A.indptr)
    assert set([1, 31, 32, 33, 64, 65, 200]) <= set(deg.tolist())
    hubs = np.flatnonzero(deg > 1)
    distinct = np.array([np.unique(part[A.indices[A.indptr[h]:A.indptr[h + 1]]]).size for h in hubs])
    assert set([127, 128, 129, 300]) <= set(distinct.tolist())
    assert all((A[h].data == 0).any() for h in hubs if deg[h] > 3), 'zero-weight edges on rows of all three routes'
    assert pw[200] > pc.CONN_CAP and pw[250] == 1 and deg[[blocked, blocked + 4, blocked + 45]].tolist() == [3, 40, 140]
    reported = np.zeros(A.shape[0], bool)
    for cap in pc.CONN_CAPS:
        room = pw + 1 <= cap
        for mode in (0, 1, 2):
            over, _, lightest = po.balance(pw, cap)
            for l in ([lightest, 200, int(np.argmax(pw))] if mode == 2 else [None]):
                (dest, gain), c = counted(po.conn, A, vw, part, pw, k, cap, mode, l)
                assert c['rows_lane'] > 0 and c['rows_wave'] >= 19 and c['rows_spill'] >= 10
                assert c['zero_only_parts'] > 0
                reported |= dest >= 0
                ok = dest >= 0
                assert (dest[ok] != part[ok]).all() and (pw[dest[ok]] + vw[ok] <= cap).all() and (gain[~ok] == 0).all()
                if mode == 0:
                    assert (dest[ok] > part[ok]).all()
                if mode == 1:
                    assert (dest[ok] < part[ok]).all()
                if mode == 2:
                    assert (pw[part[ok]] > cap).all()
                    assert (c.get('lightest_fallbacks', 0) > 0) == (l == lightest and over > 0)
                if cap == pc.CONN_CAP:
                    assert 0 < room.sum() < k and over > 0
                    # the blocked hubs: part 250 has room but only a zero-weight edge leads there
                    want = (lightest, -2) if mode == 2 and l == lightest else (-1, 0)
                    assert lightest == 250 or mode != 2
                    for h in (blocked, blocked + 4, blocked + 45):
                        assert (dest[h], gain[h]) == want, (mode, l, h)
                if cap == max(pc.CONN_CAPS) and mode < 2:
                    assert c['conn_ties'] > 0
    assert reported[hubs].mean() > 0.8, 'most hub rows report a destination under some (capacity, mode)'


def test_recount_keeps_a_candidate_whose_recounted_gain_is_positive():
    #  0 and 1 (part 0) both want part 1; 1 moves first (gain 5 > 3) and takes its edge of 4 to vertex 0 along
    A = pc.sym_from_edges(4, [0, 1, 0, 1], [1, 2, 3, 3], [4, 9, 7, 0])
    part, pw = np.array([0, 0, 1, 1]), np.array([2, 2])
    dest, gain = po.conn(A, np.ones(4), part, pw, 2, 4, 0)
    assert dest.tolist() == [1, 1, -1, -1] and gain.tolist() == [3, 5, 0, 0]
    kept, acc = po.recount(A, part, pw, gain, 4, dest)
    assert acc.tolist() == [11, 5, 0, 0] and kept.tolist() == [1, 1, -1, -1]
    # 2 and 3 in part 1 wish themselves to part 0 in an odd round: with 0 - 3 moving first the gain of 2 is gone
    A = pc.sym_from_edges(4, [2, 3, 2], [3, 0, 1], [5, 9, 6])
    dest, gain = po.conn(A, np.ones(4), part, pw, 2, 4, 1)
    assert dest.tolist() == [-1, -1, 0, 0] and gain.tolist() == [0, 0, 1, 4]
    (kept, acc), c = counted(po.recount, A, part, pw, gain, 4, dest)
    assert acc.tolist() == [0, 0, 11, 4] and c['recount_dropped'] == 0
    # a candidate whose neighbour leaves its destination first
    A = pc.sym_from_edges(5, [0, 1, 0], [1, 2, 3], [5, 9, 3])
    part, pw = np.array([0, 1, 2, 0, 2]), np.array([2, 1, 2])
    dest, gain = po.conn(A, np.ones(5), part, pw, 3, 5, 0)
    assert dest.tolist() == [1, 2, -1, -1, -1] and gain.tolist() == [2, 9, 0, 0, 0]
    (kept, acc), c = counted(po.recount, A, part, pw, gain, 5, dest)
    assert acc.tolist() == [-3, 9, 0, 0, 0] and kept.tolist() == [-1, 2, -1, -1, -1] and c['recount_dropped'] == 1


@pytest.mark.parametrize('select', [0, 1])
def test_commit_order_and_trimming(select):
    dest, gain, vw, part, pw, k, cap = pc.commit_inputs()
    out, c = counted(po.commit, dest, gain, vw, part, pw, k, cap, select)
    assert c['gains_clamped'] > 0 and c['commit_rejected'] > 0 and not (dest == 3).any()
    assert (out[dest < 0] == -1).all() and ((out == dest) | (out == -1)).all()
    T = 1 << 40
    # a sequential restatement: walk every group in (gain clamped, id) order
    want = dest.copy()
    for g in range(k):
        members = np.flatnonzero((part == g) & (dest >= 0) & (pw[part] > cap)) if select else np.flatnonzero(dest == g)
        members = sorted(members.tolist(), key=lambda v: (-max(min(int(gain[v]), T - 1), 1 - T), v))
        before = 0
        for v in members:
            if not (before < pw[g] - cap if select else before + vw[v] <= cap - pw[g]):
                want[v] = -1
            before += vw[v]
    assert np.array_equal(out, want)
    if select == 0:
        assert out[0] == -1 and out[1] == -1, 'the light vertex behind a rejected heavy one is rejected too'
        assert (out[dest == 1] == -1).all() and (out[dest == 5] == 5).sum() > 0
    else:
        outside = (dest >= 0) & (pw[part] <= cap)
        assert outside.any() and np.array_equal(out[outside], dest[outside]), 'outside an over-weight part: untouched'
        for g in (1, 4):
            assert vw[(out >= 0) & (part == g)].sum() >= pw[g] - cap, 'the prefix covers the excess'
    nothing = np.full(dest.size, -1, np.int64)
    assert np.array_equal(po.commit(nothing, gain, vw, part, pw, k, cap, select), nothing)


def test_apply_cut_balance_keep_better():
    part, pw, moved = po.apply(np.array([1, -1, 0, 2, 7]), np.array([2, 3, 4, 5, 6]), np.array([0, 0, 1, 2, 1]), np.array([5, 10, 5]), 3)
    assert part.tolist() == [1, 0, 0, 2, 1] and pw.tolist() == [7, 8, 5] and moved == 2
    A = pc.sym_from_edges(4, [0, 1, 2], [1, 2, 3], [5, 7, 9])
    assert po.cut(A, np.array([0, 0, 1, 1])) == 14 and po.cut(A, np.zeros(4, np.int64)) == 0
    assert po.balance(np.array([9, 4, 12, 4, 11]), 10) == (2, 4, 1)
    old, new = (np.array([0, 1]), np.array([3, 4])), (np.array([1, 1]), np.array([0, 7]))
    for cuts, over, undone in (([10, 12], 0, True), ([10, 12], 1, False), ([10, 10], 0, False), ([10, 8], 1, False)):
        p, w, c = po.keep_better(list(cuts), over, old[0], old[1], new[0], new[1])
        assert (p.tolist(), w.tolist()) == ((old if undone else new)[0].tolist(), (old if undone else new)[1].tolist())
        assert c == [cuts[0] if undone else cuts[1], 0]


# ---- a level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(pc.refine_cases()))
def test_refine_never_raises_the_cut_and_ends_within_capacity(name):
    A, vw, start, k, cap = pc.refine_cases()[name]
    within = po.part_weights(start, vw, k).max() <= cap
    for rounds in range(0, 9):
        (out, dest, gain), c = counted(po.refine, A, vw, start, k, cap, rounds)
        assert po.part_weights(out, vw, k).max() <= cap, 'ends within capacity'
        if within:
            assert po.cut(A, out) <= po.cut(A, start)
            assert c.get('rebalance_passes', 0) == 0
    assert po.cut(A, out) < po.cut(A, start) or not within
    assert c['commit_rejected'] > 0
    if 'k2' not in name and not name.startswith('all_in'):
        assert c['recount_dropped'] > 0 and c['conn_ties'] > 0
    if 'k2' in name:
        assert c['recount_dropped'] == 0, 'two parts, one direction a round: no neighbour moves against a candidate'
    if name.startswith('rmat'):
        assert c['rows_wave'] > 0
    if name.startswith('all_in'):
        assert not within and c['rebalance_passes'] == (3 if name.endswith('unit') else 4) and c['lightest_fallbacks'] > 0
    if name == 'two_parts_over':
        assert (po.part_weights(start, vw, k) > cap).sum() == 2


def test_refine_round_0_of_the_grid_at_k_4():
    """The figures of the first round on the 24 x 25 grid (seed 1, k = 4, random balanced start): 221 candidates, 47
    dropped by the recount, 159 rejected by the commit, 15 moved."""
    A, vw, start, k, cap = pc.refine_cases()['grid_k4_unit']
    (out, dest, gain), c = counted(po.refine, A, vw, start, k, cap, 1)
    assert ((dest >= 0).sum(), c['recount_dropped'], c['commit_rejected'], (out != start).sum()) == (221, 47, 159, 15)
    assert (gain[dest >= 0] > 0).all() and (dest[dest >= 0] > start[dest >= 0]).all(), 'round 0 moves upwards only'


def test_refine_two_neighbours_do_not_swap_for_ever():
    A = pc.sym_from_edges(8, [0, 0, 1], [1, 2, 3], [10, 1, 1])
    part = np.array([0, 1, 0, 1, 0, 1, 0, 1])
    out, dest, gain = po.refine(A, np.ones(8, np.int64), part, 2, 8, 8)
    assert dest[0] == 1 and gain[0] == 9 and dest[1] == -1
    assert out[0] == out[1] and pr.cut(A, out) <= 1 and pr.cut(A, part) == 10
    _, dest1, _ = po.refine(A, np.ones(8, np.int64), np.array([1, 0, 1, 0, 0, 1, 0, 1]), 2, 8, 1)
    assert dest1[1] == 1 and dest1[0] == -1


def test_an_undone_round():
    A, vw, part, k, cap = pc.undone_round()
    assert po.part_weights(part, vw, k).max() <= cap and po.cut(A, part) == 2 * 34
    (out, dest, gain), c = counted(po.refine, A, vw, part, k, cap, 1)
    assert dest.tolist() == [1, 2, 2, -1, -1, -1] and gain.tolist() == [4, 5, 5, 0, 0, 0]
    assert c['rounds_undone'] == 1 and c['commit_rejected'] == 1 and c['recount_dropped'] == 0
    assert np.array_equal(out, part)
    moved = part.copy()
    moved[[0, 1]] = [1, 2]   # what the round did before it was undone
    assert po.cut(A, moved) == 2 * 35


# ---- the whole call -----------------------------------------------------------------------------------------------------
def whole(A, k, value=None, nw=None):
    A = sp.csr_matrix(A)
    A.sort_indices()
    cluster = po.partition(A.indptr, A.indices, value, nw, k)
    vw = np.ones(A.shape[0], np.int64) if nw is None else nw
    assert cluster.min() >= 0 and cluster.max() < k
    assert po.part_weights(cluster, vw, k).max() <= pr.capacity(vw.sum(), k, vw.max()), 'the capacity'
    return cluster


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('kind,a,b,k', QUALITY)
def test_cut_within_twice_the_yardstick(kind, a, b, k, seed):
    if kind == 'grid':
        A, p = pr.grid(a, b, seed)
        yard = pr.grid_strips(a, b, k, p)
    else:
        A, p = pr.ring_of_cliques(a, b, seed)
        yard = pr.ring_arcs(a, b, k, p)
    got = pr.cut(A, whole(A, k))
    print('QUALITY oracle', kind, a, b, k, seed, 'cut', got, 'yardstick', pr.cut(A, yard))
    assert got <= 2 * pr.cut(A, yard)


@pytest.mark.parametrize('k', [4, 16])
def test_rmat_cut_below_random(k):
    A = pr.rmat(12, 8, seed=0)
    assert pr.cut(A, whole(A, k)) < pr.cut(A, pr.random_balanced(A.shape[0], k, 0))


WHOLE_STOP = {'rmat12_k16': 'stop_stall', 'grid96_k300': 'stop_target', 'k_above_n': 'stop_target'}


@pytest.mark.parametrize('name', sorted(pc.whole_cases()))
def test_whole_call_cases_meet_the_capacity_and_reach_their_branches(name):
    rowptr, col, value, nw, k = pc.whole_cases()[name]
    n = rowptr.size - 1
    A = sp.csr_matrix((np.ones(col.size, np.int64) if value is None else value, col, rowptr), shape=(n, n))
    po.reset_counters()
    cluster = whole(A, k, value, nw)
    c = dict(po.COUNTERS)
    assert c.get(WHOLE_STOP.get(name, 'stop_target'), 0) == 1, c
    if name in ('grid96_k300', 'k_above_n', 'rmat9_unsymmetric_self_loops'):
        assert c['levels'] == 0, 'no coarsening'
    else:
        assert c['levels'] >= 2
    if name == 'rmat12_k16':
        assert c['rows_wave'] > 0
    if n > k:
        assert pr.cut(A, cluster) < pr.cut(A, pr.random_balanced(n, k, 0))
    assert np.array_equal(cluster, po.partition(rowptr, col, value, nw, k)), 'the same input, the same cluster'


def test_trivial_calls():
    assert po.partition(np.zeros(1, np.int64), np.zeros(0, np.int64), None, None, 4).size == 0
    G = pr.grid(5, 5)[0]
    assert po.partition(G.indptr, G.indices, None, None, 1).tolist() == [0] * 25
