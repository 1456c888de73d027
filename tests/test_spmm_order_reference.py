"""The column order of the merge kernel, restated in numpy (tests/spmm_order_reference.py), held to its own claims: a
permutation of the partitions, the other partitions first and ascending, the single-row ones behind them in (key, p)
order -- and the checker itself against planted defects.  No GPU."""
import numpy as np
import pytest

from tests import spmm_order_reference as R


def skewed(M, hubs, items, seed):
    """rows of 0..7 entries and a few hub rows of several partitions' length; columns sorted inside a row"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 8, size=M)
    for r, n in hubs:
        deg[r] = n
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    N = max(M, int(deg.max()) + 1)
    col = np.concatenate([np.sort(rng.choice(N, size=int(d), replace=False)) for d in deg] + [np.zeros(0, dtype=np.int64)])
    return rowptr, col.astype(np.int64), N


CASES = [
    dict(M=300, hubs=[(0, 3 * 128 + 1)], items=128),                       # exactly two single-row partitions
    dict(M=300, hubs=[(17, 6 * 128)], items=128),                           # fewer than eight
    dict(M=1, hubs=[(0, 5000)], items=128),                                 # all but the ends
    dict(M=500, hubs=[], items=128),                                        # none
    dict(M=2000, hubs=[(3, 9000), (40, 7001), (41, 300), (1999, 4000)], items=256),
    dict(M=777, hubs=[(5, 30000), (6, 30000)], items=256),                  # equal keys are likely: ties by p
]


def build(case, seed=0):
    rowptr, col, N = skewed(case['M'], case['hubs'], case['items'], seed)
    E, M, items = col.size, case['M'], case['items']
    P = -(-(M + E) // items)
    table = R.partition_table(rowptr, E, items, P)
    single, key = R.classify(rowptr, col, table)
    return rowptr, col, table, single, key


@pytest.mark.parametrize('case', CASES)
def test_table_is_the_merge_path(case):
    rowptr, col, table, single, key = build(case)
    M, E, items = case['M'], col.size, case['items']
    assert tuple(table[0]) == (0, 0) and tuple(table[-1]) == (M, E)
    assert np.all(np.diff(table[:, 0]) >= 0) and np.all(np.diff(table[:, 1]) >= 0)
    assert np.all(table[:-1].sum(1) == np.arange(table.shape[0] - 1) * items)
    # a point never lies behind the end of the row it names, nor in front of its start
    inside = table[:, 0] < M
    assert np.all(table[inside, 1] <= rowptr[table[inside, 0] + 1]) and np.all(table[inside, 1] >= rowptr[table[inside, 0]])
    # single-row means what it says: all of the partition's items are entries of one row
    for p in np.nonzero(single)[0]:
        r, e0, e1 = table[p, 0], table[p, 1], table[p + 1, 1]
        assert e1 - e0 == items and rowptr[r] < e0 and e1 <= rowptr[r + 1]
        assert key[p] == col[e0] + col[e1 - 1]


def test_case_counts():
    counts = [int(build(c)[3].sum()) for c in CASES]
    assert counts[0] == 2 and 0 < counts[1] < 8 and counts[3] == 0
    P = build(CASES[2])[3].size
    assert counts[2] == P - 2


@pytest.mark.parametrize('case', CASES)
def test_slot_map_claims(case):
    _, _, _, single, key = build(case)
    slots = R.slot_map(single, key)
    assert slots.size == single.size
    R.check_order(slots, single, key)


def test_every_count_of_singles():
    """n_s = 0 .. 70 single-row partitions among 100, keys with many ties"""
    for n_s in range(0, 71):
        single = np.zeros(100, dtype=bool)
        single[np.arange(n_s) + 15] = True
        key = np.where(single, (np.arange(100) * 7919) % 13, R.PAD)
        R.check_order(R.slot_map(single, key), single, key)


def test_planted_defects_are_caught():
    _, _, _, single, key = build(CASES[5])
    key = key.copy()
    srt = R.sorted_singles(single, key)
    key[srt[1]] = key[srt[0]]  # a tie for certain
    good = R.slot_map(single, key)
    R.check_order(good, single, key)
    n_o = int((~single).sum())
    dropped = np.delete(good, good.size // 2)
    doubled = good.copy()
    doubled[-1] = good[0]
    tie = good.copy()  # the two partitions of the equal keys swapped: the wrong tie rule
    ia, ib = np.nonzero(good == min(srt[0], srt[1]))[0][0], np.nonzero(good == max(srt[0], srt[1]))[0][0]
    assert ib == ia + 1
    tie[ia], tie[ib] = good[ib], good[ia]
    late = good.copy()  # an "other" partition moved behind the single-row ones
    late[n_o - 1], late[-1] = good[-1], good[n_o - 1]
    unsorted = good.copy()
    unsorted[n_o:] = good[n_o:][::-1]
    for name, bad in (('dropped', dropped), ('doubled', doubled), ('tie', tie), ('late', late), ('unsorted', unsorted)):
        with pytest.raises(AssertionError):
            R.check_order(bad, single, key)


def test_engage_rule():
    assert not R.engaged(1, 10000, 1023, 10, 1024, 16384)
    assert R.engaged(1, 8192, 1024, 10, 1024, 16384)
    assert not R.engaged(1, 8193, 1024, 10, 1024, 16384)
    assert R.engaged(2, 10000, 0, 0, 1024, 16384)
    assert not R.engaged(2, 10 ** 6, 10 ** 5, 16385, 1024, 16384)
