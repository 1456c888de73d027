"""NumPy / pure-Python restatement of HGT budget sampling (torch_sparse::hgt_sample) for the tests: sets, dicts and loops,
written from the operator's semantics (docs/design/widening.md, "HGT budget sampling").  Only the deterministic parts:
columns with at most MAX_NEIGHBORS entries (no uniform sub-draw), and hops that take the whole budget.

A graph is two dicts keyed 'src__rel__dst': colptr[rel] (one column per dst node) and row[rel] (source ids)."""
import itertools

import numpy as np

MAX_NEIGHBORS = 50

# the budget vector, k and R of the selection-law tests (here and in tests/test_hgt_sample_gpu.py): every value is a sum
# of 1 / d over columns of the inputs; with k = 3 the inclusion probabilities run from 0.053 to 0.773, so R = 2000 gives
# R * pi >= 105 and R * (1 - pi) >= 453 and the normal bound applies to every candidate
LAW_BUDGETS = [1 / 2, 1 / 3, 1 / 4, 1 / 5, 1 / 2 + 1 / 3, 1 / 3 + 1 / 4, 2 / 5, 1 / 4 + 1 / 5, 1 / 6, 1 / 3 + 1 / 50]
LAW_K = 3
LAW_R = 2000


def law_bound(R, pi):
    """Five sigma of the binomial count + 1: about ten candidates per test, run on every check-in (false alarm below
    1e-4 overall)."""
    return 5.0 * np.sqrt(R * pi * (1.0 - pi)) + 1.0


def split(rel):
    src, _, dst = rel.split('__')
    return src, dst


def hgt_budget(colptr, row, lists, fresh=None, budget=None):
    """Budget update for the nodes `fresh` (type -> ids; default: everything in `lists`) given the node lists `lists`
    (type -> ids listed so far: the seen set).  Returns {type: {id: budget}} with the budget as an exact integer in
    units of 2^-32: a column of d <= MAX_NEIGHBORS entries adds floor(2^32 / d) to every unseen source."""
    fresh = lists if fresh is None else fresh
    budget = {t: {} for t in lists} if budget is None else budget
    seen = {t: set(int(v) for v in ids) for t, ids in lists.items()}
    for rel in colptr:
        src, dst = split(rel)
        cp, rw = colptr[rel], row[rel]
        for w in fresh.get(dst, ()):
            w = int(w)
            assert 0 <= w < len(cp) - 1, 'every relation into a type has one column per node of the type'
            lo, hi = int(cp[w]), int(cp[w + 1])
            d = hi - lo
            assert d <= MAX_NEIGHBORS, 'hgt_budget is deterministic only for columns of at most 50 entries'
            for j in range(lo, hi):
                v = int(rw[j])
                if v not in seen[src]:
                    budget[src][v] = budget[src].get(v, 0) + (1 << 32) // d
    return budget


def hgt_expand_det(colptr, row, inputs, types, num_hops):
    """The node SETS of every hop when every hop takes the whole budget: blocks[t] = [input list, set of hop 0, ...]."""
    lists = {t: [int(v) for v in inputs.get(t, ())] for t in types}
    blocks = {t: [list(lists[t])] for t in types}
    budget = hgt_budget(colptr, row, lists)
    for hop in range(num_hops):
        fresh = {}
        for t in types:
            fresh[t] = sorted(budget[t])
            blocks[t].append(set(fresh[t]))
            lists[t].extend(fresh[t])
            budget[t] = {}
        if hop < num_hops - 1:
            hgt_budget(colptr, row, lists, fresh, budget)
    return blocks


def hgt_assemble(colptr, row, lists, only_small=False):
    """Edges over the final node lists: per relation (row, col, edge) in dst-position order, stored order inside a
    column.  A node listed twice has its LAST position as local id.  Columns with more than MAX_NEIGHBORS entries are not
    deterministic: an assertion unless only_small, which leaves them out."""
    out = {}
    for rel in colptr:
        src, dst = split(rel)
        cp, rw = colptr[rel], row[rel]
        local = {int(v): i for i, v in enumerate(lists.get(src, ()))}
        rows, cols, edges = [], [], []
        for i, w in enumerate(lists.get(dst, ())):
            w = int(w)
            assert 0 <= w < len(cp) - 1, 'every relation into a type has one column per node of the type'
            lo, hi = int(cp[w]), int(cp[w + 1])
            if hi - lo > MAX_NEIGHBORS:
                assert only_small, 'hgt_assemble is deterministic only for columns of at most 50 entries'
                continue
            for j in range(lo, hi):
                v = int(rw[j])
                if v in local:
                    rows.append(local[v])
                    cols.append(i)
                    edges.append(j)
        out[rel] = (np.array(rows, np.int64), np.array(cols, np.int64), np.array(edges, np.int64))
    return out


def inclusion_probabilities(w, k):
    """P(candidate i is among k sequential draws without replacement, each proportional to w among what is left), by
    exact enumeration of the ordered k-tuples."""
    w = np.asarray(w, np.float64)
    P = len(w)
    total = w.sum()
    pi = np.zeros(P)
    for tup in itertools.permutations(range(P), k):
        p, rest = 1.0, total
        for i in tup:
            p *= w[i] / rest
            rest -= w[i]
        for i in tup:
            pi[i] += p
    return pi
