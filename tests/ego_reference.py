"""NumPy restatement of ego_k_hop_sample_adj (the reference's csrc/cpu/ego_sample_cpu.cpp), written from its semantics
with sets and loops like the reference.  Two halves:

  * ego_node_sets: the expansion (lines 39-76) for the inputs on which it is DETERMINISTIC -- every expanded row has
    deg <= num_neighbors (the whole row is taken), or num_neighbors <= 0 (nothing is drawn);
  * ego_assemble: n_id / root_n_id / the induced sub-graphs / the concatenation (lines 80-131) for given node sets,
    deterministic for any sets.  The GPU's own sets of a random draw go through it too.
"""
import numpy as np


def ego_node_sets(rowptr, col, idx, depth, num_neighbors, draws=None):
    """The node set of every seed: a list of sorted int64 arrays.  Raises ValueError where the reference would draw
    at random (a row with more than num_neighbors > 0 entries is expanded) -- unless a draw source says what is drawn:
    draws(hop, rowptr, frontier, k) -> (out_ptr, positions in col) (oracle/np_draws.py: ego_draws).  The frontier of
    hop 0 is idx; the one of hop l + 1 is every draw of hop l in draw order, duplicates included, each with the seed
    it was drawn for; the draws are keyed by the position in that frontier."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    if draws is not None:
        frontier = np.asarray(idx, dtype=np.int64)
        fseg = np.arange(frontier.size, dtype=np.int64)
        segs, nodes = [fseg], [frontier]
        for hop in range(depth if num_neighbors > 0 else 0):
            if frontier.size == 0:
                break
            out_ptr, pos = draws(hop, rowptr, frontier, num_neighbors)
            frontier, fseg = col[pos], np.repeat(fseg, np.diff(out_ptr))
            segs.append(fseg), nodes.append(frontier)
        seg, node = np.concatenate(segs), np.concatenate(nodes)
        return [np.unique(node[seg == g]) for g in range(len(idx))]
    sets = []
    for seed in np.asarray(idx, dtype=np.int64).tolist():
        n_id_set = {seed}
        n_ids = [seed]
        vec_start, vec_end = 0, 1
        for _ in range(depth):
            for i in range(vec_start, vec_end):  # every draw of the previous hop, duplicates included
                v = n_ids[i]
                row_start, row_end = int(rowptr[v]), int(rowptr[v + 1])
                row_count = row_end - row_start
                if row_count <= num_neighbors:
                    for e in range(row_start, row_end):
                        w = int(col[e])
                        n_id_set.add(w)
                        n_ids.append(w)
                elif num_neighbors > 0:
                    raise ValueError('node %d has %d > %d neighbours: the draw is random' % (v, row_count,
                                                                                          num_neighbors))
                # num_neighbors <= 0 and row_count > num_neighbors: no branch of the reference draws anything
            vec_start, vec_end = vec_end, len(n_ids)
        sets.append(np.array(sorted(n_id_set), dtype=np.int64))
    return sets


def ego_assemble(rowptr, col, idx, sets):
    """(rowptr, col, n_id, e_id, ptr, root_n_id) of the reference for the node sets `sets` (sorted, one per seed)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    out_rowptr, out_col, out_n_id, out_e_id = [0], [], [], []
    ptr = [0]
    root = []
    node_cumsum = 0
    for g, s in enumerate(sets):
        n_id_map = {int(v): i for i, v in enumerate(s.tolist())}
        root.append(node_cumsum + n_id_map[int(idx[g])])
        for v in s.tolist():
            for e in range(int(rowptr[v]), int(rowptr[v + 1])):
                w = int(col[e])
                if w in n_id_map:
                    out_col.append(node_cumsum + n_id_map[w])
                    out_e_id.append(e)
            out_rowptr.append(len(out_col))
        out_n_id.extend(s.tolist())
        node_cumsum += len(s)
        ptr.append(node_cumsum)
    a = lambda x: np.array(x, dtype=np.int64)  # noqa: E731
    return a(out_rowptr), a(out_col), a(out_n_id), a(out_e_id), a(ptr), a(root)


def ego_reference(rowptr, col, idx, depth, num_neighbors):
    """All six outputs where the expansion is deterministic (see ego_node_sets)."""
    return ego_assemble(rowptr, col, idx, ego_node_sets(rowptr, col, idx, depth, num_neighbors))


def hop_ball(rowptr, col, seed, depth):
    """Boolean mask of every node within `depth` hops of `seed` (following stored entries)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    ball = np.zeros(rowptr.size - 1, dtype=bool)
    ball[seed] = True
    front = np.array([seed], dtype=np.int64)
    for _ in range(depth):
        starts, lens = rowptr[front], rowptr[front + 1] - rowptr[front]
        pos = np.repeat(starts - (np.cumsum(lens) - lens), lens) + np.arange(lens.sum())
        nxt = np.unique(col[pos])
        front = nxt[~ball[nxt]]
        ball[front] = True
        if front.size == 0:
            break
    return ball
