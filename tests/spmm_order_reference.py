"""numpy restatement of the merge kernel's column order (pytorch_sparse_amd/csrc/spmm_kernels.h, section 1b; the rule
is stated in include/tsamd.h at tsamd_spmm_column_order).  Host arithmetic only.

    table       the merge-path partition: point p is the (row, entry) reached after p * items items
    single-row  table[p].row < M, table[p].entry > rowptr[row] and table[p + 1].row == row
    key         col[e0] + col[e1 - 1]
    order       every other partition first, ascending; then the single-row ones by (key, p)
"""
import numpy as np

PAD = 0xFFFFFFFF  # the key of a partition that is not single-row


def partition_table(rowptr, E, items, P):
    """[P + 1, 2] int64 (row, entry): on diagonal d the path has passed every row r with rowptr[r + 1] + r + 1 <= d."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    M = rowptr.size - 1
    d = np.minimum(np.arange(P + 1, dtype=np.int64) * items, M + E)
    ends = rowptr[1:] + np.arange(1, M + 1, dtype=np.int64)  # strictly increasing
    row = np.searchsorted(ends, d, side='right').astype(np.int64)
    return np.stack([row, d - row], axis=1)


def classify(rowptr, col, table):
    """(single [P] bool, key [P] int64; the key of a partition that is not single-row is PAD)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    M = rowptr.size - 1
    r0, e0, r1, e1 = table[:-1, 0], table[:-1, 1], table[1:, 0], table[1:, 1]
    inside = r0 < M
    start = rowptr[np.minimum(r0, M - 1)] if M > 0 else np.zeros_like(r0)
    single = inside & (e0 > start) & (r1 == r0)
    key = np.full(r0.size, PAD, dtype=np.int64)
    key[single] = col[e0[single]] + col[e1[single] - 1]
    return single, key


def sorted_singles(single, key):
    """the single-row partitions by (key, p)"""
    p = np.nonzero(single)[0]
    return p[np.lexsort((p, key[p]))]


def slot_map(single, key):
    """slot -> partition [P]: the other partitions in ascending order, then the single-row ones by (key, p).  Slots of
    four share a workgroup and consecutive workgroups go to the XCDs in turn: all of them walk the sorted list together."""
    return np.concatenate([np.nonzero(~single)[0], sorted_singles(single, key)]).astype(np.int64)


def engaged(mode, P, n_s, max_bucket, min_singles, bucket_max):
    """what the device decides: forced, or enough single-row partitions; never with an oversized bucket"""
    if max_bucket > bucket_max:
        return False
    return mode == 2 or (n_s >= min_singles and n_s * 8 >= P)


def check_order(slots, single, key):
    """The claims of the rule, on any slot map; raises AssertionError with the first one that fails."""
    P = single.size
    slots = np.asarray(slots, dtype=np.int64)
    assert slots.size == P and np.array_equal(np.sort(slots), np.arange(P)), 'not a permutation of the partitions'
    n_o = int((~single).sum())
    assert np.array_equal(slots[:n_o], np.nonzero(~single)[0]), 'the other partitions do not come first, ascending'
    walked = slots[n_o:]
    k = key[walked]
    ok = (k[1:] > k[:-1]) | ((k[1:] == k[:-1]) & (walked[1:] > walked[:-1]))
    assert bool(ok.all()), 'single-row partitions out of (key, p) order'
