"""The graphs of the reverse Cuthill-McKee tests (tests/test_rcm_oracle.py on the CPU, tests/test_rcm_gpu.py on the GPU):
symmetric CSR matrices (rowptr, col) as int64 numpy arrays with sorted rows and no repeated entries.  Node ids are
shuffled with a fixed seed where the table says so.  Not collected by pytest."""
import functools

import numpy as np
import scipy.sparse as sp


def _sym(n, r, c, diag=()):
    r, c, d = np.asarray(r, np.int64), np.asarray(c, np.int64), np.asarray(diag, np.int64)
    rows = np.concatenate([r, c, d])
    cols = np.concatenate([c, r, d])
    A = sp.csr_matrix((np.ones(rows.size, np.int8), (rows, cols)), shape=(n, n))  # repeated pairs are summed away
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64)


def _shuffle(n, r, c, seed):
    p = np.random.default_rng(seed).permutation(n)
    return p[np.asarray(r, np.int64)], p[np.asarray(c, np.int64)]


def path():
    i = np.arange(299)
    return _sym(300, i, i + 1)


def star():
    """Hub 0 with 5000 leaves; the first seed is a leaf, so the hub owns the other 4999 in one level."""
    return _sym(5001, np.zeros(5000, np.int64), np.arange(1, 5001))


def two_hubs():
    """Hubs 0 and 1, adjacent, sharing the 2000 leaves 2..2001; 1000 outer nodes hang off three of the first 1500 leaves
    each.  Both hubs and 496 leaves carry their diagonal, which raises scipy's degree by two (the entry, and one more).
    The seed is a bare leaf, so both hubs stand in one frontier and contend for the other 1999 leaves."""
    leaves = np.arange(2, 2002)
    outer = np.arange(2002, 3002)
    att = (np.arange(3000) * 7) % 1500 + 2  # every one of the first 1500 leaves twice
    r = np.concatenate([[0], np.zeros(2000, np.int64), np.ones(2000, np.int64), np.repeat(outer, 3)])
    c = np.concatenate([[1], leaves, leaves, att])
    diag = np.concatenate([[0, 1], np.arange(2, 2002, 4)[:496]])
    return _sym(3002, r, c, diag)


def grid():
    """40 x 40 four-neighbour grid, ids shuffled."""
    idx = np.arange(1600).reshape(40, 40)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return _sym(1600, *_shuffle(1600, r, c, 1))


def many_components():
    """700 isolated nodes, 400 pairs, 200 triangles and a connected 500-node random blob, ids shuffled."""
    rng = np.random.default_rng(2)
    pr = 700 + 2 * np.arange(400)
    tr = 1500 + 3 * np.arange(200)
    b0 = 2100
    chain = np.arange(499)  # a random spanning tree keeps the blob in one piece
    parent = rng.integers(0, chain + 1)
    extra = rng.integers(0, 500, (2, 1500))
    r = np.concatenate([pr, tr, tr + 1, tr, b0 + chain + 1, b0 + extra[0]])
    c = np.concatenate([pr + 1, tr + 1, tr + 2, tr + 2, b0 + parent, b0 + extra[1]])
    keep = r != c
    return _sym(2600, *_shuffle(2600, r[keep], c[keep], 3))


def skewed(seed=4):
    """R-MAT-like: 40 000 draws over 2^12 nodes, quadrant probabilities (0.57, 0.19, 0.19, 0.05), diagonals kept."""
    rng = np.random.default_rng(seed)
    r = np.zeros(40_000, np.int64)
    c = np.zeros(40_000, np.int64)
    for _ in range(12):
        q = rng.random(40_000)
        r = 2 * r + (q >= 0.76)
        c = 2 * c + (((q >= 0.57) & (q < 0.76)) | (q >= 0.95))
    return _sym(4096, r, c)


def uniform():
    """30 000 uniform draws over a 3000 x 3000 matrix, symmetrised: the graph of test_select_gpu.py's RCM test."""
    key = np.unique(np.random.default_rng(12).integers(0, 3000 * 3000, 30_000))
    return _sym(3000, key // 3000, key % 3000)


def empty5():
    return np.zeros(6, np.int64), np.zeros(0, np.int64)


def one_with_diagonal():
    return np.array([0, 1], np.int64), np.zeros(1, np.int64)


def no_nodes():
    return np.zeros(1, np.int64), np.zeros(0, np.int64)


# name -> (builder, nodes, levels, components); the last two as scipy's search visits them (None: degenerate, the
# oracle's own figures are used)
CASES = {
    'path': (path, 300, 300, 1),
    'star': (star, 5001, 3, 1),
    'two_hubs': (two_hubs, 3002, 4, 1),
    'grid': (grid, 1600, 79, 1),
    'many_components': (many_components, 2600, 1907, 1301),
    'skewed': (skewed, 4096, 1008, 1002),
    'uniform': (uniform, 3000, 5, 1),
    'empty5': (empty5, 5, None, None),
    'one_with_diagonal': (one_with_diagonal, 1, None, None),
    'no_nodes': (no_nodes, 0, None, None),
}


@functools.lru_cache(maxsize=None)
def get(name):
    """(rowptr, col) of a case, built once per process; the arrays are shared, do not write to them."""
    rowptr, col = CASES[name][0]()
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return rowptr, col
