"""A numpy / scipy restatement of the HIP partitioner (csrc/partition.hip, csrc/ops_partition.cpp), written from
docs/design/partition.md: one function per C-ABI stage, each returning exactly the arrays the device writes, then the
round loop of a level and the whole call.  Everything is int64 arithmetic, a stable sort and sums whose order does not
matter, so the device result must equal this one element for element (tests/test_partition_exact_gpu.py).  Not
collected by pytest; tests/test_partition_oracle.py holds it to the invariants the design promises.

A graph is a scipy CSR matrix with sorted indices and int64 data; explicit zeros are entries (a zero-weight edge is an
edge for matching and the BFS, but gives no connectivity to a part).  COUNTERS records which branches a run took."""
import collections

import numpy as np
import scipy.sparse as sp

MASK = 0xFFFFFFFF
LANE_ROW = 32          # rows up to this many entries take a lane
SLOTS = 128            # distinct parts a wave's LDS table holds
GAIN_CLAMP = 1 << 40
COARSEN_PER_PART, COARSEN_FLOOR, MATCH_ROUNDS, REFINE_ROUNDS, MAX_LEVELS = 64, 512, 4, 8, 64

COUNTERS = collections.Counter()


def reset_counters():
    COUNTERS.clear()


def i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return sp.csr_matrix((A.data.astype(np.int64), A.indices.astype(np.int64), A.indptr.astype(np.int64)), shape=A.shape)


def coo_of(A):
    """(row, col, w) of the CSR entries in storage order."""
    return np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)), A.indices.astype(np.int64), A.data


# ---- the tie hash ---------------------------------------------------------------------------------------------------
def tie_hash(round_, id_):
    """32-bit multiply-xorshift mix of (round, id) in Python ints."""
    x = (round_ * 0x9E3779B1 + id_ * 0x85EBCA77) & MASK
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & MASK
    x ^= x >> 12
    x = (x * 0x297A2D39) & MASK
    x ^= x >> 15
    return x


def tie_hash_array(round_, ids):
    """tie_hash over an array of ids (uint64 arithmetic masked to 32 bits) -> int64."""
    m = np.uint64(MASK)
    x = (np.uint64(round_ * 0x9E3779B1 & MASK) + (np.asarray(ids).astype(np.uint64) & m) * np.uint64(0x85EBCA77)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & m
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & m
    x ^= x >> np.uint64(15)
    return x.astype(np.int64)


# ---- working graph / contraction ------------------------------------------------------------------------------------
def _from_entries(n, r, c, w):
    """CSR of the entry list with r == c dropped and duplicates summed; a sum of zero stays an entry."""
    keep = r != c
    r, c, w = r[keep], c[keep], w[keep]
    key = r * max(n, 1) + c
    order = np.argsort(key, kind='stable')
    key, w = key[order], w[order]
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if key.size else np.zeros(0, np.int64)
    ukey = key[start]
    uw = np.add.reduceat(w, start) if key.size else np.zeros(0, np.int64)
    ur, uc = ukey // max(n, 1), ukey % max(n, 1)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(ur, minlength=n))]).astype(np.int64)
    return sp.csr_matrix((i64(uw), i64(uc), indptr), shape=(n, n))


def level0(rowptr, col, value=None):
    """A + A^T of the CSR input with self-loops dropped and duplicates summed (a symmetric input doubles)."""
    rowptr, col = i64(rowptr), i64(col)
    n = rowptr.size - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    w = np.ones(col.size, np.int64) if value is None else i64(value)
    return _from_entries(n, np.concatenate([row, col]), np.concatenate([col, row]), np.concatenate([w, w]))


def contract(A, vw, cmap, n_c):
    """(cmap[r], cmap[c], w) without r == c, duplicates summed, and the summed vertex weights."""
    r, c, w = coo_of(A)
    cmap = i64(cmap)
    vw_c = np.zeros(n_c, np.int64)
    np.add.at(vw_c, cmap, i64(vw))
    return _from_entries(n_c, cmap[r], cmap[c], w), vw_c


# ---- matching -------------------------------------------------------------------------------------------------------
def leaders(match):
    """(cmap, n_c): the leader of a pair is the smaller id, cmap the exclusive scan of the leader flags."""
    n = match.size
    lead = (match < 0) | (np.arange(n) < match)
    rank = np.cumsum(lead) - lead
    cmap = np.where(lead, rank, rank[np.where(match >= 0, match, 0)])
    return i64(cmap), int(lead.sum())


def match_rounds(A, vw, cap, rounds):
    """Yields (match, cmap, n_c) after 0, 1, ..., `rounds` handshake rounds."""
    A, vw = csr(A), i64(vw)
    n = A.shape[0]
    r, u, w = coo_of(A)
    match = np.full(n, -1, np.int64)
    yield (match.copy(),) + leaders(match)
    for rnd in range(rounds):
        ok = (match[r] < 0) & (match[u] < 0) & (u != r) & (vw[r] + vw[u] <= cap)
        rr, uu, ww = r[ok], u[ok], w[ok]
        order = np.lexsort((-uu, tie_hash_array(rnd, uu), ww, rr))  # the best (w, hash, -id) of a row comes last
        rr, uu, ww = rr[order], uu[order], ww[order]
        last = np.flatnonzero(np.concatenate([rr[1:] != rr[:-1], [True]])) if rr.size else np.zeros(0, np.int64)
        prop = np.full(n, -1, np.int64)
        prop[rr[last]] = uu[last]
        # branch counters: rows whose best weight is shared (the hash decides), rows whose heaviest free neighbour is
        # too heavy for the cap, proposing rows of the wave kernel
        tied = last[(last > 0) & (rr[last - 1] == rr[last]) & (ww[last - 1] == ww[last])]
        COUNTERS['match_ties'] += int(tied.size)
        chosen = np.full(n, -1, np.int64)
        chosen[rr[last]] = ww[last]
        heavy = (match[r] < 0) & (match[u] < 0) & (u != r) & (vw[r] + vw[u] > cap) & (w > chosen[r])
        COUNTERS['match_cap_blocked'] += int(np.unique(r[heavy]).size)
        COUNTERS['match_rows_wave'] += int((np.diff(A.indptr)[rr[last]] > LANE_ROW).sum())
        COUNTERS['match_ties_wave'] += int((np.diff(A.indptr)[rr[tied]] > LANE_ROW).sum())
        v = np.flatnonzero(prop >= 0)
        v = v[prop[prop[v]] == v]
        match[v] = prop[v]
        yield (match.copy(),) + leaders(match)


def match(A, vw, cap, rounds):
    out = None
    for out in match_rounds(A, vw, cap, rounds):
        pass
    return out


# ---- initial partition ----------------------------------------------------------------------------------------------
def bfs_keys(A):
    """(component, level) of every vertex: the first search starts at the vertex of minimum (degree, id) among those
    with edges, later ones at the smallest unvisited id; vertices without edges form the last component n, level 0."""
    A = csr(A)
    n = A.shape[0]
    deg = np.diff(A.indptr)
    comp = np.where(deg == 0, n, -1).astype(np.int64)
    level = np.zeros(n, np.int64)
    COUNTERS['bfs_isolated'] += int((deg == 0).sum())
    if not (deg > 0).any():
        return comp, level
    COUNTERS['bfs_seed_ties'] += int((deg == deg[deg > 0].min()).sum() > 1)
    seed = int(np.lexsort((np.arange(n), np.where(deg > 0, deg, deg.max() + 1)))[0])
    c, scan = 0, 0
    while True:
        comp[seed] = c
        frontier, lv = np.array([seed], np.int64), 0
        while frontier.size:
            idx = A[frontier].indices
            nxt = np.unique(idx[comp[idx] < 0])
            lv += 1
            comp[nxt] = c
            level[nxt] = lv
            frontier = nxt
        while scan < n and comp[scan] >= 0:
            scan += 1
        if scan == n:
            COUNTERS['bfs_components'] += c + 1
            return comp, level
        seed, c = scan, c + 1


def initial(A, vw, k):
    """part of every vertex: stable order by (component, level, id), part = floor((2 prefix + w) k / (2 W))."""
    vw = i64(vw)
    n = vw.size
    comp, level = bfs_keys(A)
    order = np.lexsort((np.arange(n), level, comp))
    ws = vw[order]
    prefix = np.cumsum(ws) - ws
    W = int(ws.sum())
    COUNTERS['initial_zero_total'] += int(W == 0)
    p = ((2 * prefix + ws) * k) // (2 * W) if W > 0 else (np.arange(n, dtype=np.int64) * k) // max(n, 1)
    part = np.empty(n, np.int64)
    part[order] = np.clip(p, 0, k - 1)
    return part


# ---- refinement -----------------------------------------------------------------------------------------------------
def part_weights(part, vw, k):
    pw = np.zeros(k, np.int64)
    np.add.at(pw, i64(part), i64(vw))
    return pw


def count_routes(A, part):
    """Rows by the route their connectivity takes: a lane (up to 32 entries), a wave's table (longer, up to 128
    distinct parts among the entries, the own part included), the spill list (more)."""
    A = csr(A)
    r, c, _ = coo_of(A)
    deg = np.diff(A.indptr)
    k = int(part.max()) + 1 if part.size else 1
    distinct = np.bincount(np.unique(r * k + part[c]) // k, minlength=A.shape[0])
    COUNTERS['rows_lane'] += int((deg <= LANE_ROW).sum())
    COUNTERS['rows_wave'] += int(((deg > LANE_ROW) & (distinct <= SLOTS)).sum())
    COUNTERS['rows_spill'] += int(((deg > LANE_ROW) & (distinct > SLOTS)).sum())


def conn(A, vw, part, pw, k, cap, mode, lightest=None):
    """(dest, gain) of every vertex.  A part is adjacent when the connectivity to it is positive.  mode 0 / 1: the
    best adjacent part above / below the own one with room for the vertex (largest connectivity, then smallest id),
    reported when the gain is positive or the own part is over capacity.  mode 2: only vertices of over-weight parts,
    any direction, and the lightest part (gain = -c_own) when no adjacent part has room."""
    A, vw, part, pw = csr(A), i64(vw), i64(part), i64(pw)
    n = A.shape[0]
    count_routes(A, part)
    P = sp.csr_matrix((np.ones(n, np.int64), (np.arange(n), part)), shape=(n, k))
    C = (A @ P).tocoo()
    v, p, c = C.row.astype(np.int64), C.col.astype(np.int64), C.data.astype(np.int64)
    pos = c > 0
    v, p, c = v[pos], p[pos], c[pos]
    own = part[v]
    r_, c_, _ = coo_of(A)
    reached = r_[part[c_] != part[r_]] * k + part[c_][part[c_] != part[r_]]
    COUNTERS['zero_only_parts'] += int(np.unique(reached).size - (p != own).sum())  # reached by zero weights alone
    c_own = np.zeros(n, np.int64)
    c_own[v[p == own]] = c[p == own]
    ok = (p != own) & (pw[p] + vw[v] <= cap)
    if mode == 0:
        ok &= p > own
    elif mode == 1:
        ok &= p < own
    v, p, c = v[ok], p[ok], c[ok]
    order = np.lexsort((p, -c, v))
    v, p, c = v[order], p[order], c[order]
    first = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]])) if v.size else np.zeros(0, np.int64)
    dest = np.full(n, -1, np.int64)
    gain = np.zeros(n, np.int64)
    dest[v[first]] = p[first]
    gain[v[first]] = c[first] - c_own[v[first]]
    nxt = first[first + 1 < v.size] + 1
    COUNTERS['conn_ties'] += int(((v[nxt] == v[nxt - 1]) & (c[nxt] == c[nxt - 1])).sum())  # the smaller id decides
    heavy = pw[part] > cap
    if mode == 2:
        dest[~heavy] = -1
        if lightest is not None:
            l = int(lightest)
            fall = heavy & (dest < 0) & (part != l) & (pw[l] + vw <= cap)
            dest[fall] = l
            gain[fall] = -c_own[fall]
            COUNTERS['lightest_fallbacks'] += int(fall.sum())
    else:
        dest[(dest >= 0) & ~((gain > 0) | heavy)] = -1
    gain[dest < 0] = 0
    return dest, gain


def recount(A, part, pw, gain, cap, dest):
    """(dest, acc): acc = the gain of a candidate with every neighbour that moves first (higher gain, then smaller id)
    already at its destination; a candidate stays iff acc > 0 or its own part is over capacity."""
    A, part, pw, gain, dest = csr(A), i64(part), i64(pw), i64(gain), i64(dest).copy()
    r, c, w = coo_of(A)
    live = dest[r] >= 0
    r, c, w = r[live], c[live], w[live]
    first = (dest[c] >= 0) & ((gain[c] > gain[r]) | ((gain[c] == gain[r]) & (c < r)))
    pc = np.where(first, dest[c], part[c])
    acc = np.zeros(part.size, np.int64)
    np.add.at(acc, r, w * (pc == dest[r]) - w * (pc == part[r]))
    drop = (dest >= 0) & ~((acc > 0) | (pw[part] > cap))
    COUNTERS['recount_dropped'] += int(drop.sum())
    dest[drop] = -1
    return dest, acc


def commit(dest, gain, vw, part, pw, k, cap, select):
    """dest with the rejected candidates set to -1.  Order: (group, gain descending, id); `before` = the weight of
    everything earlier in the group, rejected vertices included.  select 0: group = destination, accepted iff
    before + w <= cap - pw[group]; select 1: group = the own part when it is over capacity, accepted iff
    before < pw[group] - cap (a candidate outside such a part keeps its destination)."""
    dest, gain, vw, part, pw = i64(dest).copy(), i64(gain), i64(vw), i64(part), i64(pw)
    n = dest.size
    g = dest.copy()
    if select:
        g = np.where(g >= 0, np.where(pw[part] > cap, part, -1), g)
    x = np.clip(gain, 1 - GAIN_CLAMP, GAIN_CLAMP - 1)
    COUNTERS['gains_clamped'] += int(((x != gain) & (g >= 0)).sum())
    key_row = np.where(g < 0, k, g)
    key_col = np.where(g < 0, 0, GAIN_CLAMP - x)
    order = np.lexsort((np.arange(n), key_col, key_row))
    gs, ws = key_row[order], vw[order]
    prefix = np.cumsum(ws) - ws
    start = np.searchsorted(gs, gs, side='left')
    before = prefix - prefix[start] if n else prefix
    in_group = gs < k
    gg = np.where(in_group, gs, 0)
    ok = (before < pw[gg] - cap) if select else (before + ws <= cap - pw[gg])
    rejected = order[in_group & ~ok]
    COUNTERS['commit_rejected'] += int(rejected.size)
    dest[rejected] = -1
    return dest


def apply(dest, vw, part, pw, k):
    """(part, pw, moved) after the accepted moves."""
    dest, vw, part, pw = i64(dest), i64(vw), i64(part).copy(), i64(pw).copy()
    go = (dest >= 0) & (dest < k) & (dest != part)
    np.add.at(pw, part[go], -vw[go])
    np.add.at(pw, dest[go], vw[go])
    part[go] = dest[go]
    return part, pw, int(go.sum())


def cut(A, part):
    """Twice the cut weight (every edge is stored in both directions)."""
    r, c, w = coo_of(csr(A))
    part = i64(part)
    return int(w[part[r] != part[c]].sum())


def balance(pw, cap):
    """(parts over capacity, smallest part weight, smallest id of a part of that weight)."""
    pw = i64(pw)
    return int((pw > cap).sum()), int(pw.min()), int(np.argmin(pw))


def keep_better(cuts, over, part_old, pw_old, part, pw):
    """(part, pw, cuts): a round that started within capacity (over == 0) and raised the cut is undone; cuts[0] then
    keeps the old cut, else takes the new one; cuts[1] = 0."""
    undo = cuts[1] > cuts[0] and over == 0
    if undo:
        return i64(part_old).copy(), i64(pw_old).copy(), [cuts[0], 0]
    return i64(part).copy(), i64(pw).copy(), [cuts[1], 0]


def refine(A, vw, part, k, cap, rounds):
    """The loop of one level -> (part, dest of round 0, gain of round 0); the last two are empty for rounds == 0."""
    A, vw, part = csr(A), i64(vw), i64(part).copy()
    pw = part_weights(part, vw, k)
    cuts = [cut(A, part), 0]
    first = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    idle, moved, rnd = 0, 0, 0
    while rnd < rounds and idle < 2:
        over = balance(pw, cap)[0]
        dest, gain = conn(A, vw, part, pw, k, cap, rnd & 1)
        if rnd == 0:
            first = (dest.copy(), gain.copy())
        dest, _ = recount(A, part, pw, gain, cap, dest)
        dest = commit(dest, gain, vw, part, pw, k, cap, 0)
        part_old, pw_old = part, pw
        part, pw, moved = apply(dest, vw, part, pw, k)
        cuts[1] = cut(A, part)
        if cuts[1] > cuts[0] and over == 0:
            COUNTERS['rounds_undone'] += 1
        part, pw, cuts = keep_better(cuts, over, part_old, pw_old, part, pw)
        idle = idle + 1 if moved == 0 else 0
        rnd += 1
    for pass_ in range(4 * k + 16):
        over, _, lightest = balance(pw, cap)
        if over == 0 or (pass_ > 0 and moved == 0):
            break
        COUNTERS['rebalance_passes'] += 1
        dest, gain = conn(A, vw, part, pw, k, cap, 2, lightest)
        dest = commit(dest, gain, vw, part, pw, k, cap, 1)
        dest = commit(dest, gain, vw, part, pw, k, cap, 0)
        part, pw, moved = apply(dest, vw, part, pw, k)
    return part, first[0], first[1]


# ---- the whole call -------------------------------------------------------------------------------------------------
def capacity(W, k, w_max):
    return (103 * int(W)) // (100 * int(k)) + int(w_max)


def partition(rowptr, col, value, node_weight, k):
    """cluster of partition / partition2 / mt_partition."""
    rowptr = i64(rowptr)
    n = rowptr.size - 1
    if n == 0 or k == 1:
        return np.zeros(n, np.int64)
    vw = np.ones(n, np.int64) if node_weight is None else i64(node_weight)
    W, w_max = int(vw.sum()), int(vw.max())
    cap = capacity(W, k, w_max)
    target = max(COARSEN_PER_PART * k, COARSEN_FLOOR)
    match_cap = max(w_max, (3 * W) // (2 * target))
    levels, cmaps = [(level0(rowptr, col, value), vw)], []
    stop = 'stop_target'
    while levels[-1][0].shape[0] > target:
        if len(levels) >= MAX_LEVELS:
            stop = 'stop_levels'
            break
        A, w = levels[-1]
        _, cmap, n_c = match(A, w, match_cap, MATCH_ROUNDS)
        if n_c * 100 > A.shape[0] * 95:
            stop = 'stop_stall'
            break
        levels.append(contract(A, w, cmap, n_c))
        cmaps.append(cmap)
    COUNTERS['levels'] += len(levels) - 1
    COUNTERS[stop] += 1
    part = initial(levels[-1][0], levels[-1][1], k)
    part = refine(levels[-1][0], levels[-1][1], part, k, cap, REFINE_ROUNDS)[0]
    for l in range(len(levels) - 2, -1, -1):
        part = refine(levels[l][0], levels[l][1], part[cmaps[l]], k, cap, REFINE_ROUNDS)[0]
    return part
