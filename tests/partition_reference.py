"""Helpers of the partition tests (numpy / scipy only, not collected): graph builders with a seeded random relabelling
of the vertex ids -- so a partitioner that cuts id ranges gains nothing --, cut and part weights on the symmetrised
graph, the contraction oracle, and the explicit feasible partitions the cut is measured against."""
import numpy as np
import scipy.sparse as sp


def _relabel(edges, n, seed):
    """Symmetric 0/1 CSR of the undirected edge list [2, m] with ids shuffled by `seed` (None: as they are); also
    returns the shuffle p (new id of old vertex v = p[v])."""
    p = np.arange(n) if seed is None else np.random.RandomState(seed).permutation(n)
    r, c = p[edges[0]], p[edges[1]]
    A = sp.coo_matrix((np.ones(2 * r.size, np.int64), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n))
    A = A.tocsr()
    A.sum_duplicates()
    A.data[:] = 1
    A.sort_indices()
    return A, p


def grid(h, w, seed=None):
    idx = np.arange(h * w).reshape(h, w)
    edges = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()]),
                            np.stack([idx[:-1].ravel(), idx[1:].ravel()])], 1)
    return _relabel(edges, h * w, seed)


def ring_of_cliques(count, size, seed=None):
    """`count` cliques of `size` vertices, one bridge edge between consecutive cliques (last vertex -> first vertex)."""
    i, j = np.triu_indices(size, 1)
    base = np.arange(count) * size
    inner = np.stack([(base[:, None] + i[None]).ravel(), (base[:, None] + j[None]).ravel()])
    bridge = np.stack([base + size - 1, np.roll(base, -1)])
    return _relabel(np.concatenate([inner, bridge], 1), count * size, seed)


def rmat(scale, edge_factor, seed=0, abc=(0.57, 0.19, 0.19)):
    """Small R-MAT (directed entries, duplicates merged, ids shuffled): 0/1 CSR, NOT symmetric."""
    rs = np.random.RandomState(seed)
    n, m = 1 << scale, (1 << scale) * edge_factor
    r, c = np.zeros(m, np.int64), np.zeros(m, np.int64)
    a, b, cc = abc
    for bit in range(scale):
        u = rs.rand(m)
        r |= (u >= a + b).astype(np.int64) << bit
        c |= (((u >= a) & (u < a + b)) | (u >= a + b + cc)).astype(np.int64) << bit
    p = rs.permutation(n)
    A = sp.coo_matrix((np.ones(m, np.int64), (p[r], p[c])), shape=(n, n)).tocsr()
    A.sum_duplicates()
    A.data[:] = 1
    A.sort_indices()
    return A


def symmetrise(A):
    """The undirected graph of A without self-loops, int64 weights: an edge weighs the larger of its two directions, so
    a symmetric A is left as it is.  (The partitioner sums the two directions; for a symmetric A that doubles every
    weight alike and changes no cut ratio.)"""
    A = sp.csr_matrix(A).astype(np.int64)
    S = A.maximum(A.T).tocsr()
    S.setdiag(0)
    S.eliminate_zeros()
    S.sort_indices()
    return S


def cut(A, cluster):
    """Weight of the edges of the symmetrised graph whose ends lie in different parts (every edge once)."""
    S = symmetrise(A).tocoo()
    cluster = np.asarray(cluster)
    return int(S.data[cluster[S.row] != cluster[S.col]].sum()) // 2


def part_weights(cluster, k, vw=None):
    cluster = np.asarray(cluster)
    vw = np.ones(cluster.size, np.int64) if vw is None else np.asarray(vw, np.int64)
    out = np.zeros(k, np.int64)
    np.add.at(out, cluster, vw)
    return out


def capacity(W, k, w_max):
    """floor(1.03 W / k) + w_max in exact integer arithmetic."""
    return (103 * int(W)) // (100 * int(k)) + int(w_max)


def contract_oracle(A, vw, cmap):
    """P^T A P without its diagonal (P[v, cmap[v]] = 1) and the summed vertex weights -> (csr int64, vw_c int64)."""
    A = sp.csr_matrix(A).astype(np.int64)
    cmap = np.asarray(cmap)
    n, nc = A.shape[0], int(cmap.max()) + 1 if cmap.size else 0
    P = sp.csr_matrix((np.ones(n, np.int64), (np.arange(n), cmap)), shape=(n, nc))
    C = (P.T @ A @ P).tocsr()
    C.setdiag(0)
    C.eliminate_zeros()
    C.sum_duplicates()
    C.sort_indices()
    vw_c = np.zeros(nc, np.int64)
    np.add.at(vw_c, cmap, np.asarray(vw, np.int64))
    return C.astype(np.int64), vw_c


def random_balanced(n, k, seed):
    """A seeded random partition with part sizes within one of n / k."""
    return np.random.RandomState(seed).permutation(n) % k


def grid_strips(h, w, k, p):
    """Row strips of the h x w grid (cut (k - 1) w): original vertex (i, j) -> part floor(i k / h), in shuffled ids."""
    part_of_row = (np.arange(h) * k) // h
    out = np.empty(h * w, np.int64)
    out[p] = np.repeat(part_of_row, w)
    return out


def ring_arcs(count, size, k, p):
    """Arcs of whole cliques of the ring (cut k): clique q -> part floor(q k / count), in shuffled ids."""
    out = np.empty(count * size, np.int64)
    out[p] = np.repeat((np.arange(count) * k) // count, size)
    return out
