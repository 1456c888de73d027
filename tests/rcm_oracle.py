"""numpy restatement of scipy.sparse.csgraph.reverse_cuthill_mckee(symmetric_mode=True) as a level-synchronous search
(docs/design/rcm.md), in two forms that csrc/rcm.hip and its host driver follow:

  rcm_sorted   every level sorts its new nodes by (position of the owning frontier node, degree, id)
  rcm_scan     the nodes are relabelled once by their rank in stable (degree, id) order and the rows re-sorted by the new
               column ids; a level is then owner-by-min, a 0 / 1 flag per frontier entry, an exclusive scan of the flags
               in (frontier position, adjacency) order and a write at the scanned offset -- no sort inside the loop

Both return (order, levels, components); perm = order[::-1].  `levels` counts every non-empty frontier, seeds included.
Not collected by pytest (no test_ prefix); tests/test_rcm_oracle.py checks it against scipy."""
import numpy as np


def degrees(rowptr, col):
    """scipy's degree: the row length, plus one where the row holds its own diagonal (counted once)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = rowptr.size - 1
    deg = np.diff(rowptr)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    has_diag = np.zeros(n, bool)
    has_diag[row[row == col]] = True
    return deg + has_diag


def degree_dtype(n, nnz):
    """The index dtype scipy gives a CSR matrix of this size, which is the dtype its degree array is sorted in."""
    return np.int32 if max(n, nnz) < 2 ** 31 else np.int64


def seed_order(rowptr, col):
    """The order in which scipy tries the nodes as component seeds: numpy's DEFAULT argsort of the degrees.  That sort
    is not stable, so ties depend on the numpy build; only the same call on the same dtype reproduces it."""
    deg = degrees(rowptr, col)
    return np.argsort(deg.astype(degree_dtype(deg.size, len(col)))).astype(np.int64)


def stable_seed_order(rowptr, col):
    return np.argsort(degrees(rowptr, col), kind='stable').astype(np.int64)


def _frontier_entries(rowptr, col, order, lo, hi):
    """Entries of the rows of order[lo:hi] in (frontier position, adjacency) order -> (owner position, column)."""
    u = order[lo:hi]
    length = rowptr[u + 1] - rowptr[u]
    start = np.cumsum(length) - length
    total = int(length.sum())
    p = np.repeat(np.arange(lo, hi, dtype=np.int64), length)
    k = np.arange(total, dtype=np.int64) - np.repeat(start, length) + np.repeat(rowptr[u], length)
    return p, col[k]


def rcm_sorted(rowptr, col, seeds):
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = rowptr.size - 1
    deg = degrees(rowptr, col)
    order = np.empty(n, np.int64)
    visited = np.zeros(n, bool)
    count = levels = components = 0
    for s in np.asarray(seeds, np.int64):
        if visited[s]:
            continue
        visited[s] = True
        order[count] = s
        lo, hi = count, count + 1
        count += 1
        components += 1
        while hi > lo:
            levels += 1
            p, j = _frontier_entries(rowptr, col, order, lo, hi)
            keep = ~visited[j]  # a self loop is never new: its node is in the frontier, hence visited
            p, j = p[keep], j[keep]
            srt = np.lexsort((p, j))  # by node, then owner position: the first of each node is its smallest owner
            p, j = p[srt], j[srt]
            first = np.ones(j.size, bool)
            first[1:] = j[1:] != j[:-1]
            p, j = p[first], j[first]
            nxt = j[np.lexsort((j, deg[j], p))]
            visited[nxt] = True
            order[count:count + nxt.size] = nxt
            lo, hi = hi, hi + nxt.size
            count = hi
    return order, levels, components


def relabel(rowptr, col):
    """-> (rowptr', col', by_rank): node r of the relabelled graph is by_rank[r], rows sorted by the new ids."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = rowptr.size - 1
    by_rank = np.argsort(degrees(rowptr, col), kind='stable').astype(np.int64)
    rank = np.empty(n, np.int64)
    rank[by_rank] = np.arange(n, dtype=np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    r2, c2 = rank[row], rank[col]
    srt = np.lexsort((c2, r2))
    r2, c2 = r2[srt], c2[srt]
    rowptr2 = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r2, minlength=n), out=rowptr2[1:])
    return rowptr2, c2, by_rank, rank


def rcm_scan(rowptr, col, seeds, trace=None):
    """trace (a list, optional): receives (frontier nodes, frontier entries) of every level, for choosing capacities."""
    rowptr2, col2, by_rank, rank = relabel(rowptr, col)
    n = rowptr2.size - 1
    big = np.iinfo(np.int64).max
    pos = np.full(n, -1, np.int64)
    owner = np.full(n, big, np.int64)
    order = np.empty(n, np.int64)
    hi = levels = components = 0
    for s in rank[np.asarray(seeds, np.int64)]:
        if pos[s] >= 0:
            continue
        pos[s] = hi
        order[hi] = s
        lo, hi = hi, hi + 1
        components += 1
        while hi > lo:
            levels += 1
            p, j = _frontier_entries(rowptr2, col2, order, lo, hi)
            if trace is not None:
                trace.append((hi - lo, j.size))
            dup = np.zeros(j.size, bool)
            dup[1:] = (j[1:] == j[:-1]) & (p[1:] == p[:-1])  # a repeated entry of a sorted row counts once
            cand = (pos[j] < 0) & ~dup
            np.minimum.at(owner, j[cand], p[cand])  # claim
            flag = cand & (owner[j] == p)
            off = np.cumsum(flag) - flag  # exclusive scan in (frontier position, adjacency) order
            q = hi + off[flag]
            pos[j[flag]] = q
            order[q] = j[flag]
            lo, hi = hi, hi + int(flag.sum())
    return by_rank[order], levels, components


def rcm(rowptr, col, seeds=None):
    """-> (perm, levels, components) with scipy's seeds unless given."""
    if seeds is None:
        seeds = seed_order(rowptr, col)
    order, levels, components = rcm_sorted(rowptr, col, seeds)
    return order[::-1].copy(), levels, components
