"""Inputs shared by tests/test_partition_oracle.py (CPU: the oracle alone, and that every case reaches the branch it is
named for) and tests/test_partition_exact_gpu.py (the device against the oracle).  numpy / scipy only, generated from
seeds, not collected."""
import numpy as np
import scipy.sparse as sp

from tests import partition_reference as pr


def sym_from_edges(n, r, c, w=None):
    """Symmetric CSR of the undirected edges; zero weights stay entries."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    w = np.ones(len(r), np.int64) if w is None else np.asarray(w, np.int64)
    A = sp.csr_matrix((np.concatenate([w, w]) + 1, (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    A.data -= 1  # (weights went in one too large so that a zero is never dropped on the way; no edge is listed twice)
    return A.astype(np.int64)


def reweighted(A, lo, hi, seed):
    """The symmetric 0/1 graph A with one random weight in [lo, hi] per undirected edge."""
    U = sp.triu(A, 1).tocoo()
    return sym_from_edges(A.shape[0], U.row, U.col, np.random.RandomState(seed).randint(lo, hi + 1, U.nnz))


# ---- matching: name -> (A, vw, cap) ---------------------------------------------------------------------------------
def match_hubs():
    """Hubs of degree 31 ... 200.  Five leaves spread over the row tie for the heaviest eligible weight 50 (the hash
    decides, through the wave reduction on the long rows); the single heaviest leaf (weight 100, the last of the row)
    weighs 4 and is too heavy for the cap of 4 next to the hub's 1."""
    rs = np.random.RandomState(5)
    r, c, w, vw = [], [], [], []
    n = 0
    for deg in (31, 32, 33, 63, 64, 65, 200):
        hub, leaves = n, np.arange(n + 1, n + 1 + deg)
        n += deg + 1
        x = rs.randint(1, 10, deg)
        x[np.linspace(0, deg - 2, 5).astype(int)] = 50
        x[-1] = 100
        lw = rs.randint(1, 3, deg)
        lw[-1] = 4
        r += [hub] * deg
        c += leaves.tolist()
        w += x.tolist()
        vw += [1] + lw.tolist()
    return sym_from_edges(n, r, c, w), np.array(vw, np.int64), 4


def match_cases():
    grid = pr.grid(24, 25, seed=1)[0]
    rmat = reweighted(pr.symmetrise(pr.rmat(9, 6, seed=1)), 1, 3, seed=2)
    return {
        'unit_grid': (grid, np.ones(600, np.int64), 2),
        'rmat9': (rmat, np.random.RandomState(3).randint(1, 5, 512).astype(np.int64), 5),
        'hubs': match_hubs(),
    }


# ---- initial partition: name -> (A, vw, k) --------------------------------------------------------------------------
def initial_cases():
    grid = pr.grid(12, 13, seed=0)[0]
    blocks = [pr.grid(h, w)[0] for h, w in ((3, 4), (5, 5), (2, 9), (6, 3), (4, 4))] + [sp.csr_matrix((3, 3), dtype=np.int64)]
    five = sp.block_diag(blocks).tocsr()
    p = np.random.RandomState(4).permutation(five.shape[0])
    five = five[p][:, p].tocsr()
    path = sym_from_edges(6, [0, 1, 2, 3, 4], [1, 2, 3, 4, 5])
    return {
        'grid_k5': (grid, np.random.RandomState(0).randint(1, 4, 156).astype(np.int64), 5),
        'grid_k7': (grid, np.random.RandomState(1).randint(1, 4, 156).astype(np.int64), 7),
        'five_components': (five, np.ones(five.shape[0], np.int64), 4),
        'k_above_n': (path, np.ones(6, np.int64), 10),  # the path's two ends also tie for the minimum degree
        'no_edges': (sp.csr_matrix((9, 9), dtype=np.int64), np.arange(1, 10, dtype=np.int64), 3),
        'zero_weights': (grid, np.zeros(156, np.int64), 5),
        'seed_tie': (sym_from_edges(5, [3, 0, 1, 2], [0, 1, 2, 4]), np.ones(5, np.int64), 3),  # ends 3 and 4: degree 1
    }


# ---- connectivity ---------------------------------------------------------------------------------------------------
CONN_K, CONN_CAP = 301, 24
CONN_CAPS = (CONN_CAP, 40, 10 ** 6)  # some parts full and some over weight, fewer, every part has room


def conn_graph():
    """Stars whose hubs are the rows under test -> (A, vw, part).  Degrees 1 (every leaf), 31, 32, 33, 64, 65, 200 over
    few parts; hubs touching exactly 127, 128, 129 and 300 distinct parts (the own part is one of them); weights in
    0..3, so zero-weight edges and ties in connectivity sit on every route.  Three `blocked` hubs (a lane's, a wave's, a
    spilled row) weigh CONN_CAP - 1 in an over-weight part: the only part with room for them holds one leaf of weight 1
    behind a zero-weight edge."""
    rs = np.random.RandomState(11)
    r, c, w, vw, part = [], [], [], [], []
    n = 0

    def star(leaf_parts, weights, hub_part, hub_vw=None):
        nonlocal n
        deg = len(leaf_parts)
        hub = n
        r.extend([hub] * deg)
        c.extend(range(n + 1, n + 1 + deg))
        w.extend(weights)
        vw.extend([rs.randint(1, 4) if hub_vw is None else hub_vw] + rs.randint(1, 4, deg).tolist())
        part.extend([hub_part] + list(leaf_parts))
        n += deg + 1
        return hub

    for deg in (1, 31, 32, 33, 64, 65, 200):   # few parts: ties in connectivity, the smaller part id wins
        for hub_part in (0, 3, 6):
            star(rs.randint(0, 7, deg), rs.randint(0, 4, deg), hub_part)
    for distinct, deg in ((127, 180), (128, 180), (129, 180), (300, 420), (129, 129)):
        for hub_part in (0, 150, 299):
            others = rs.permutation(np.setdiff1d(np.arange(CONN_K), [hub_part]))[:distinct - 1]
            lp = np.concatenate([[hub_part], others])   # the distinct parts of the row, the own part among them
            lp = np.concatenate([lp, rs.choice(lp[:distinct // 3], deg - distinct)])
            star(rs.permutation(lp), rs.randint(0, 4, deg), hub_part)
    # blocked hubs: own part 200 is over weight through them; every part they reach with a positive weight holds 2 at
    # least and is full for a vertex of weight CONN_CAP - 1; part 250 weighs 1 in all, behind a zero-weight edge
    first_blocked = n
    for deg in (3, 40, 140):
        hub = star([200, 250] + list(range(2, deg)), [2, 0] + rs.randint(1, 4, deg - 2).tolist(), 200, hub_vw=CONN_CAP - 1)
        vw[hub + 3:hub + 1 + deg] = [2] * (deg - 2)
    vw, part = np.array(vw, np.int64), np.array(part, np.int64)
    vw[part == 250] = 0
    vw[first_blocked + 2] = 1
    A = sym_from_edges(n, r, c, w)
    return A, vw, part, first_blocked


# ---- commit: explicit arrays ----------------------------------------------------------------------------------------
def commit_inputs():
    """(dest, gain, vw, part, pw, k, cap): k = 6 with group 3 empty; gains at and beyond the clamp 2^40 and runs of
    equal gains; group 0 has room for 4 and is led by a vertex of weight 5, behind it one of weight 1 (rejected too:
    `before` counts the rejected weight); parts 1 and 4 are over capacity for select = 1."""
    rs = np.random.RandomState(21)
    T = 1 << 40
    special = [T - 1, T, T + 5, -(T - 1), -T, -(T + 5), 7, 7, 7, 0, -3, 12]
    n, k, cap = 96, 6, 20
    dest = rs.choice([-1, 0, 1, 2, 4, 5], n)
    gain = np.array([special[i % len(special)] for i in rs.permutation(n)], np.int64)
    vw = rs.randint(1, 6, n).astype(np.int64)
    part = rs.randint(0, k, n).astype(np.int64)
    part = np.where(part == dest, (part + 1) % k, part)
    pw = np.array([16, 27, 11, 20, 31, 2], np.int64)
    # group 0: ids 0, 1 lead it by gain; 0 is too heavy for the room of 4, 1 would fit alone
    dest[[0, 1]] = 0
    gain[[0, 1]] = [T + 100, T + 50]
    vw[[0, 1]] = [5, 1]
    part[[0, 1]] = 2
    return dest.astype(np.int64), gain, vw, part, pw, k, cap


# ---- refinement: name -> (A, vw, start, k, cap) ---------------------------------------------------------------------
def refine_cases():
    out = {}
    for graph in ('grid', 'rmat'):
        A = pr.grid(24, 25, seed=1)[0] if graph == 'grid' else pr.symmetrise(pr.rmat(9, 6, seed=1))
        n = A.shape[0]
        for k in (2, 4, 7):
            for weights in ('unit', 'random'):
                vw = np.ones(n, np.int64) if weights == 'unit' else np.random.RandomState(k).randint(1, 5, n).astype(np.int64)
                out['%s_k%d_%s' % (graph, k, weights)] = (A, vw, pr.random_balanced(n, k, seed=k), k,
                                                          pr.capacity(vw.sum(), k, vw.max()))
    A = pr.grid(16, 16, seed=2)[0]
    for weights in ('unit', 'random'):
        vw = np.ones(256, np.int64) if weights == 'unit' else np.random.RandomState(9).randint(1, 5, 256).astype(np.int64)
        out['all_in_part_0_%s' % weights] = (A, vw, np.zeros(256, np.int64), 4, pr.capacity(vw.sum(), 4, vw.max()))
    A = pr.grid(24, 25, seed=1)[0]
    skew = np.random.RandomState(6).choice(4, 600, p=[0.45, 0.45, 0.05, 0.05]).astype(np.int64)
    out['two_parts_over'] = (A, np.ones(600, np.int64), skew, 4, pr.capacity(600, 4, 1))
    return out


def undone_round():
    """A round 0 that raises the cut from 34 to 35 and is undone -> (A, vw, part, k, cap).
    X = 0 (part 0) gains 4 by going to part 1: edges N1 10 and S 4 there, N2 10 at home.  N1 = 1 (part 1, gain 5 to
    part 2) and N2 = 2 (part 0, weight 3, gain 5 to part 2) both move first.  The recount of X sees N1 gone (-10) and N2
    gone (+10) and keeps X; the commit takes N1 and rejects N2 (part 2 has room for 3, N1 came first), so X moves and
    loses 6 while N1 gains 5."""
    #                        X-N1 X-N2 X-S N1-Q N2-T
    A = sym_from_edges(6, [0, 0, 0, 1, 2], [1, 2, 3, 4, 5], [10, 10, 4, 5, 15])
    vw = np.array([1, 1, 3, 1, 1, 1], np.int64)
    part = np.array([0, 1, 0, 1, 2, 2], np.int64)
    return A, vw, part, 3, 5


# ---- the whole call: name -> (rowptr, col, value, node_weight, k) ---------------------------------------------------
def planted_clusters():
    rs = np.random.RandomState(0)
    n = 1024
    planted = rs.permutation(n) // 16
    order = np.argsort(planted, kind='stable').reshape(64, 16)
    i, j = np.triu_indices(16, 1)
    keep = rs.rand(64, i.size) < 0.4
    hr, hc = order[:, i][keep], order[:, j][keep]
    lr, lc = rs.randint(0, n, 6 * n), rs.randint(0, n, 6 * n)
    ok = planted[lr] != planted[lc]
    A = sp.coo_matrix((np.concatenate([np.full(hr.size, 100), np.ones(ok.sum(), np.int64)] * 2),
                          (np.concatenate([hr, lr[ok], hc, lc[ok]]), np.concatenate([hc, lc[ok], hr, lr[ok]]))),
                         shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A.astype(np.int64)


def whole_cases():
    def case(A, k, value=False, nw=None):
        A = sp.csr_matrix(A)
        A.sort_indices()
        return (A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.int64) if value else None, nw, k)

    path = sym_from_edges(7, [0, 1, 2, 3, 4, 5], [1, 2, 3, 4, 5, 6])
    return {
        'grid64_k2': case(pr.grid(64, 64, 0)[0], 2),
        'grid64_k8': case(pr.grid(64, 64, 0)[0], 8),
        'grid48x80_k5': case(pr.grid(48, 80, 0)[0], 5),
        'ring256x8_k4': case(pr.ring_of_cliques(256, 8, 0)[0], 4),
        'rmat12_k16': case(pr.rmat(12, 8, seed=0), 16),
        'planted_weighted': case(planted_clusters(), 4, value=True),
        'grid30x31_node_weights': case(pr.grid(30, 31, seed=5)[0], 6, nw=np.random.RandomState(0).randint(1, 6, 930).astype(np.int64)),
        'rmat9_unsymmetric_self_loops': case(pr.rmat(9, 4, seed=3) + sp.eye(512, dtype=np.int64, format='csr'), 4),
        'grid96_k300': case(pr.grid(96, 96, 0)[0], 300),
        'k_above_n': case(path, 20),
    }
