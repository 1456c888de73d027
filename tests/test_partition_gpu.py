"""The HIP partitioner (csrc/partition.hip, docs/design/partition.md) on the GPU: each phase through its tsamd:: op
against invariants and exact oracles, then SparseTensor.partition end to end -- the reference's output contract, the
capacity floor(1.03 W / k) + w_max, reproducibility, and the cut against explicit balanced partitions built here
(row strips of a grid, whole-clique arcs of a ring of cliques): at most twice theirs.  A seeded random balanced
partition lands at 13x to 3000x on these graphs and a working multilevel scheme near 1x, so the factor separates the
two without asking for METIS-grade hill climbing."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import pytorch_sparse_amd as ts
from tests import partition_reference as pr

pytestmark = pytest.mark.gpu
OPS = torch.ops.tsamd


def csr_dev(A, dev, weight=True):
    A = sp.csr_matrix(A)
    A.sort_indices()
    rowptr = torch.from_numpy(A.indptr.astype(np.int64)).to(dev)
    col = torch.from_numpy(A.indices.astype(np.int64)).to(dev)
    w = torch.from_numpy(A.data.astype(np.int64)).to(dev) if weight else None
    return rowptr, col, w


def t64(x, dev):
    return torch.from_numpy(np.asarray(x, np.int64)).to(dev)


def sym_from_edges(n, r, c, w=None):
    w = np.ones(len(r), np.int64) if w is None else np.asarray(w, np.int64)
    A = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    A.sort_indices()
    return A


# ---- matching -----------------------------------------------------------------------------------------------------------
def run_match(A, vw, cap, dev, rounds=4):
    rowptr, col, w = csr_dev(A, dev)
    match, cmap, n_c = OPS.partition_match(rowptr, col, w, t64(vw, dev), cap, rounds)
    match, cmap, n_c = match.cpu().numpy(), cmap.cpu().numpy(), int(n_c.item())
    n = A.shape[0]
    D = sp.csr_matrix(A)
    for v in np.nonzero(match >= 0)[0]:
        m = match[v]
        assert m != v and D[v, m] != 0, 'a matched pair is an edge'
        assert match[m] == v, 'the match is mutual (so no vertex is in two pairs)'
        assert vw[v] + vw[m] <= cap, 'the weight cap holds'
    leader = (match < 0) | (np.arange(n) < match)
    rank = np.cumsum(leader) - leader
    want = np.where(leader, rank, rank[np.where(match >= 0, match, 0)])
    assert n_c == int(leader.sum()) and np.array_equal(cmap, want)
    assert np.array_equal(np.unique(cmap), np.arange(n_c))
    return match


def test_match_path_of_two(dev):
    A = sym_from_edges(2, [0], [1])
    assert run_match(A, np.ones(2, np.int64), 2, dev).tolist() == [1, 0]
    assert run_match(A, np.ones(2, np.int64), 1, dev).tolist() == [-1, -1]  # the cap forbids the only pair


def test_match_star_and_isolated(dev):
    n = 201 + 5  # hub 0, leaves 1..200, five isolated vertices
    A = sym_from_edges(n, np.zeros(200, np.int64), np.arange(1, 201))
    match = run_match(A, np.ones(n, np.int64), 2, dev)
    assert match[0] >= 1 and (match[1:201] >= 0).sum() == 1 and (match[201:] < 0).all()


def test_match_clique_of_equal_weights(dev):
    n = 300
    i, j = np.triu_indices(n, 1)
    match = run_match(sym_from_edges(n, i, j), np.ones(n, np.int64), 2, dev)
    assert (match >= 0).sum() >= 2


def test_match_rows_around_a_wave(dev):
    """Hubs of degree 63 / 64 / 65 whose heaviest edge is the LAST of the row: the hub and that leaf propose to each
    other in round 0, whatever lane or loop tail holds the edge."""
    r, c, w, hubs, best = [], [], [], [], []
    n = 0
    for deg in (63, 64, 65, 31, 32, 33):
        hub, leaves = n, np.arange(n + 1, n + 1 + deg)
        n += deg + 1
        r += [hub] * deg
        c += leaves.tolist()
        w += list(range(1, deg)) + [1000]
        hubs.append(hub)
        best.append(leaves[-1])
    match = run_match(sym_from_edges(n, r, c, w), np.ones(n, np.int64), 2, dev)
    assert match[hubs].tolist() == best


def test_match_heaviest_edge_of_distinct_weights(dev):
    rs = np.random.RandomState(0)
    n = 500
    M = sp.triu(sp.random(n, n, 0.02, random_state=rs, data_rvs=lambda s: np.ones(s)), 1).tocoo()
    w = rs.permutation(M.nnz) + 1
    A = sym_from_edges(n, M.row, M.col, w)
    match = run_match(A, np.ones(n, np.int64), 2, dev)
    e = int(np.argmax(w))
    assert match[M.row[e]] == M.col[e]


# ---- contraction --------------------------------------------------------------------------------------------------------
def run_contract(A, vw, cmap, dev):
    rowptr, col, w = csr_dev(A, dev)
    n_c = int(np.max(cmap)) + 1
    got = [x.cpu().numpy() for x in OPS.partition_contract(rowptr, col, w, t64(vw, dev), t64(cmap, dev), n_c)]
    C, vw_c = pr.contract_oracle(A, vw, cmap)
    assert np.array_equal(got[0], C.indptr) and np.array_equal(got[1], C.indices)
    assert got[2].dtype == np.int64 and np.array_equal(got[2], C.data) and np.array_equal(got[3], vw_c)
    return C


def test_contract_drops_the_self_loop(dev):
    A = sym_from_edges(4, [0, 1, 2], [1, 2, 3], [5, 7, 9])
    C = run_contract(A, [1, 2, 3, 4], [0, 0, 1, 2], dev)
    assert C.nnz == 4 and C.diagonal().sum() == 0


def test_contract_sums_parallel_edges(dev):
    A = sym_from_edges(4, [0, 0, 1, 1, 0], [2, 3, 2, 3, 1], [1, 2, 3, 4, 100])
    C = run_contract(A, [1, 1, 1, 1], [0, 0, 1, 1], dev)
    assert C.nnz == 2 and C[0, 1] == 10


def test_contract_int64_weights(dev):
    big = 1 << 40
    A = sym_from_edges(6, [0, 0, 1, 1, 4, 2], [2, 3, 2, 3, 5, 3], [big + 1, big + 2, big + 3, big + 4, big, 7])
    C = run_contract(A, [big, 1, 2, 3, 4, 5], [0, 0, 1, 1, 2, 2], dev)
    assert C[0, 1] == 4 * big + 10


def test_contract_random(dev):
    A, _ = pr.grid(9, 11, seed=3)
    A = A.astype(np.int64)
    A.data[:] = np.random.RandomState(1).randint(1, 9, A.nnz)
    A = pr.symmetrise(sp.triu(A, 1))
    rs = np.random.RandomState(2)
    run_contract(A, rs.randint(1, 5, 99), rs.permutation(99) % 40, dev)


# ---- initial partition --------------------------------------------------------------------------------------------------
def run_initial(A, vw, k, dev):
    rowptr, col, _ = csr_dev(A, dev)
    part = OPS.partition_initial(rowptr, col, t64(vw, dev), k).cpu().numpy()
    assert part.shape == (A.shape[0],) and part.min() >= 0 and part.max() < k
    pw = pr.part_weights(part, k, vw)
    assert np.abs(pw - vw.sum() / k).max() <= vw.max(), (pw, vw.sum() / k)
    return part


def test_initial_connected(dev):
    A, _ = pr.grid(12, 13, seed=0)
    run_initial(A, np.random.RandomState(0).randint(1, 4, 156).astype(np.int64), 5, dev)
    run_initial(A, np.ones(156, np.int64), 7, dev)


def test_initial_five_components_and_isolated(dev):
    blocks = [pr.grid(h, w)[0] for h, w in ((3, 4), (5, 5), (2, 9), (6, 3), (4, 4))] + [sp.csr_matrix((3, 3), dtype=np.int64)]
    A = sp.block_diag(blocks).tocsr()
    p = np.random.RandomState(4).permutation(A.shape[0])
    A = A[p][:, p].tocsr()
    part = run_initial(A, np.ones(A.shape[0], np.int64), 4, dev)
    assert len(np.unique(part)) == 4


def test_initial_more_parts_than_vertices(dev):
    A = sym_from_edges(6, [0, 1, 2, 3, 4], [1, 2, 3, 4, 5])
    run_initial(A, np.ones(6, np.int64), 10, dev)


# ---- refinement ---------------------------------------------------------------------------------------------------------
def run_refine(A, vw, part, k, cap, dev, rounds=8):
    rowptr, col, w = csr_dev(A, dev)
    out, dest, gain = OPS.partition_refine(rowptr, col, w, t64(vw, dev), t64(part, dev), k, cap, rounds)
    return out.cpu().numpy(), dest.cpu().numpy(), gain.cpu().numpy()


@pytest.mark.parametrize('graph', ['grid', 'rmat'])
def test_refine_never_raises_the_cut_and_keeps_the_capacity(dev, graph):
    A = pr.grid(24, 25, seed=1)[0] if graph == 'grid' else pr.symmetrise(pr.rmat(9, 6, seed=1))
    n = A.shape[0]
    for k in (2, 4, 7):
        vw = np.ones(n, np.int64)
        start = pr.random_balanced(n, k, seed=k)
        cap = pr.capacity(n, k, 1)
        assert pr.part_weights(start, k).max() <= cap
        out, _, _ = run_refine(A, vw, start, k, cap, dev)
        print(graph, k, 'cut', pr.cut(A, start), '->', pr.cut(A, out))
        assert pr.cut(A, out) <= pr.cut(A, start)
        assert pr.cut(A, out) < pr.cut(A, start), 'a random start always leaves positive gains'
        assert pr.part_weights(out, k).max() <= cap


def test_refine_two_neighbours_do_not_swap_for_ever(dev):
    """u (part 0) and v (part 1) share a heavy edge and hold light ones at home: each prefers the other's part.  Moving
    both keeps the heavy edge cut; the direction rule lets only one of them go in a round."""
    #            u  v  a  b + padding so that both parts have room
    A = sym_from_edges(8, [0, 0, 1], [1, 2, 3], [10, 1, 1])
    part = np.array([0, 1, 0, 1, 0, 1, 0, 1])
    out, dest, gain = run_refine(A, np.ones(8, np.int64), part, 2, 8, dev, rounds=8)
    assert dest[0] == 1 and gain[0] == 9  # round 0 moves upwards only
    assert out[0] == out[1] and pr.cut(A, out) <= 1 and pr.cut(A, part) == 10


def test_refine_connectivity_of_long_rows_equals_numpy(dev):
    """Hubs of 5000 / 100 / 20 neighbours spread over 300 / 40 / 7 parts: more parts than the LDS table holds (the
    scratch table), a wave's LDS table, a lane's loop.  Round 0 reports (best part above the own one, gain)."""
    rs = np.random.RandomState(0)
    k, r, c, w, part, hubs = 301, [], [], [], [], []
    n = 0
    for deg, parts in ((5000, 300), (100, 40), (20, 7)):
        hub, leaves = n, np.arange(n + 1, n + 1 + deg)
        n += deg + 1
        hubs.append(hub)
        r += [hub] * deg
        c += leaves.tolist()
        w += rs.randint(1, 6, deg).tolist()
        part += [0] + (rs.randint(0, parts, deg) + (0 if parts < 300 else 1)).tolist()
    part, w = np.array(part), np.array(w)
    part[1:4] = 0  # some weight at home
    A = sym_from_edges(n, r, c, w)
    _, dest, gain = run_refine(A, np.ones(n, np.int64), part, k, n, dev, rounds=1)
    for hub in hubs:
        lo, hi = A.indptr[hub], A.indptr[hub + 1]
        conn = np.bincount(part[A.indices[lo:hi]], weights=A.data[lo:hi], minlength=k).astype(np.int64)
        other = conn.copy()
        other[0] = -1
        best = int(np.argmax(other))  # first maximum = smallest part id
        want = (best, conn[best] - conn[0]) if conn[best] > conn[0] else (-1, 0)  # only a positive gain is reported
        assert (dest[hub], gain[hub]) == want, hub
    assert dest[hubs[0]] > 0


def test_refine_over_weight_start_ends_within_capacity(dev):
    A, _ = pr.grid(16, 16, seed=2)
    cap = pr.capacity(256, 4, 1)
    out, _, _ = run_refine(A, np.ones(256, np.int64), np.zeros(256, np.int64), 4, cap, dev)
    assert pr.part_weights(out, 4).max() <= cap


# ---- end to end ---------------------------------------------------------------------------------------------------------
def sparse_tensor(A, dev, value=None):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return ts.SparseTensor(rowptr=torch.from_numpy(A.indptr.astype(np.int64)).to(dev),
                           col=torch.from_numpy(A.indices.astype(np.int64)).to(dev),
                           value=None if value is None else torch.as_tensor(value).to(dev),
                           sparse_sizes=A.shape, is_sorted=True)


def partition_checked(A, k, dev, vw=None, value=None, **kw):
    """SparseTensor.partition + the output contract of torch_sparse/metis.py:69-75 and the capacity -> cluster."""
    src = sparse_tensor(A, dev, value)
    n = A.shape[0]
    out, partptr, perm = src.partition(k, **kw)
    assert perm.dtype == torch.long and np.array_equal(np.sort(perm.cpu().numpy()), np.arange(n))
    pp = partptr.cpu().numpy()
    assert pp.shape == (k + 1,) and pp[0] == 0 and pp[-1] == n and (np.diff(pp) >= 0).all()
    want = ts.permute(src, perm)
    for a, b in zip(out.csr(), want.csr()):
        assert (a is None and b is None) or torch.equal(a, b)
    cluster = np.empty(n, np.int64)
    cluster[perm.cpu().numpy()] = np.repeat(np.arange(k), np.diff(pp))
    assert (np.diff(cluster[perm.cpu().numpy()]) >= 0).all()
    vw = np.ones(n, np.int64) if vw is None else np.asarray(vw, np.int64)
    pw = pr.part_weights(cluster, k, vw)
    assert pw.max() <= pr.capacity(vw.sum(), k, vw.max()), (pw.max(), pr.capacity(vw.sum(), k, vw.max()))
    return cluster


def test_partition_through_the_ops(dev):
    A, _ = pr.grid(20, 20, seed=0)
    rowptr, col, _ = csr_dev(A, dev)
    a = torch.ops.torch_sparse.partition(rowptr, col, None, 4, False)
    b = torch.ops.torch_sparse.partition2(rowptr, col, None, None, 4, False)
    c = torch.ops.torch_sparse.mt_partition(rowptr, col, None, None, 4, True, 8)
    assert a.dtype == torch.long and a.device == rowptr.device and a.shape == (400,)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert pr.part_weights(a.cpu().numpy(), 4).max() <= pr.capacity(400, 4, 1)


def test_partition_contract_options_and_reproducibility(dev):
    A, _ = pr.grid(30, 31, seed=5)
    n = A.shape[0]
    first = partition_checked(A, 6, dev)
    assert np.array_equal(first, partition_checked(A, 6, dev)), 'two calls, the same cluster bit for bit'
    assert np.array_equal(first, partition_checked(A, 6, dev, recursive=True))
    rs = np.random.RandomState(0)
    nw_int = rs.randint(1, 6, n)
    partition_checked(A, 6, dev, vw=nw_int, node_weight=torch.from_numpy(nw_int))
    nw_float = torch.from_numpy(rs.choice([0.5, 1.0, 1.5, 3.0], n))
    partition_checked(A, 6, dev, vw=ts.metis.weight2metis(nw_float.clone()).numpy(), node_weight=nw_float)
    partition_checked(A, 6, dev, vw=np.bincount(A.indices, minlength=n), balance_edge=True)
    src = sparse_tensor(A, dev)
    out, partptr, perm = src.partition(1)
    assert out is src and partptr.tolist() == [0, n] and torch.equal(perm.cpu(), torch.arange(n))
    with pytest.raises(ValueError, match='balance_edge'):
        src.partition(2, node_weight=torch.ones(n), balance_edge=True)


def test_partition_more_parts_than_vertices(dev):
    A = sym_from_edges(7, [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6])
    cluster = partition_checked(A, 20, dev)
    assert cluster.max() < 20


def test_partition_unsymmetric_input_with_self_loops(dev):
    A = pr.rmat(9, 4, seed=3) + sp.eye(512, dtype=np.int64, format='csr')
    cluster = partition_checked(A.tocsr(), 4, dev)
    assert pr.cut(A, cluster) < pr.cut(A, pr.random_balanced(512, 4, 0))


def test_partition_weighted_follows_the_heavy_edges(dev):
    """64 planted clusters of 16 vertices joined inside by edges of weight 100, scattered light edges between them:
    without `weighted` the planted clusters are invisible."""
    rs = np.random.RandomState(0)
    n = 1024
    planted = rs.permutation(n) // 16
    order = np.argsort(planted, kind='stable').reshape(64, 16)
    i, j = np.triu_indices(16, 1)
    keep = rs.rand(64, i.size) < 0.4
    hr, hc = order[:, i][keep], order[:, j][keep]
    lr, lc = rs.randint(0, n, 6 * n), rs.randint(0, n, 6 * n)
    ok = planted[lr] != planted[lc]
    A = sym_from_edges(n, np.concatenate([hr, lr[ok]]), np.concatenate([hc, lc[ok]]),
                       np.concatenate([np.full(hr.size, 100), np.ones(ok.sum(), np.int64)]))
    A.sum_duplicates()
    plain = partition_checked(A, 4, dev, value=A.data.astype(np.float32))
    heavy = partition_checked(A, 4, dev, value=A.data.astype(np.float32), weighted=True)
    heavy_int = partition_checked(A, 4, dev, value=A.data.astype(np.int64), weighted=True)
    print('weighted cut: plain', pr.cut(A, plain), 'weighted', pr.cut(A, heavy), pr.cut(A, heavy_int))
    assert not np.array_equal(plain, heavy)
    assert pr.cut(A, heavy) < pr.cut(A, plain)


def test_partition_many_parts(dev):
    """k = 300 on a 96 x 96 grid: no coarsening (n < 64 k), hundreds of parts around every refinement kernel."""
    A, _ = pr.grid(96, 96, seed=0)
    cluster = partition_checked(A, 300, dev)
    got, rand = pr.cut(A, cluster), pr.cut(A, pr.random_balanced(96 * 96, 300, 0))
    print('k=300 cut', got, 'random', rand)
    assert got < rand


QUALITY = ([('grid', 64, 64, k) for k in (2, 4, 8)] + [('grid', 48, 80, k) for k in (3, 5)] +
           [('ring', 256, 8, k) for k in (2, 4, 8)] + [('ring', 64, 32, k) for k in (4, 8)])


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('kind,a,b,k', QUALITY)
def test_cut_within_twice_the_yardstick(dev, kind, a, b, k, seed):
    """The yardstick is made of whole rows (whole cliques), so it is balanced to one row (clique): every part has at
    most ceil(a / k) of them.  That is exact on all cases but the 48 x 80 grid at k = 5, where 48 rows split 10, 10, 9,
    10, 9 and a strip of 800 vertices sits 8 above the capacity floor(1.03 * 3840 / 5) + 1 = 792 that our own result
    must (and is checked to) meet.  The bar stays twice the strips' cut (k - 1) w there as everywhere: a partition
    that does meet the capacity has to break a row, so the bar asks no less than one taken from it would."""
    if kind == 'grid':
        A, p = pr.grid(a, b, seed)
        yard = pr.grid_strips(a, b, k, p)
        assert pr.cut(A, yard) == (k - 1) * b
    else:
        A, p = pr.ring_of_cliques(a, b, seed)
        yard = pr.ring_arcs(a, b, k, p)
        assert pr.cut(A, yard) == k
    assert pr.part_weights(yard, k).max() == -(-a // k) * b, 'the yardstick is balanced to one row / clique'
    cluster = partition_checked(A, k, dev)
    got = pr.cut(A, cluster)
    print('QUALITY', kind, a, b, k, seed, 'cut', got, 'yardstick', pr.cut(A, yard), 'ratio %.3f' % (got / pr.cut(A, yard)))
    assert got <= 2 * pr.cut(A, yard)


@pytest.mark.parametrize('k', [4, 16])
def test_rmat_cut_below_random(dev, k):
    A = pr.rmat(12, 8, seed=0)
    cluster = partition_checked(A, k, dev)
    got, rand = pr.cut(A, cluster), pr.cut(A, pr.random_balanced(A.shape[0], k, 0))
    print('QUALITY rmat12 k', k, 'cut', got, 'random', rand, 'ratio %.3f' % (got / rand))
    assert got < rand
