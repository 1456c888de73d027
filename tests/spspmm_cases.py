"""Seeded generator of wide hypersparse products for the SpSpMM tests: A (m x k) * B (k x N) with k = 4096, a few
hundred thousand entries in B and column ids up to N - 1 -- only the ids are large, so N = 2^32 - 2 costs the same
device memory as N = 2^20.  numpy only, deterministic from (N, lg_range, seed).  Test infrastructure, not a conftest.

Rows of B: empty | 1-3 entries | "spread" (12-20 columns over the whole [0, N); a quarter of them share a pool of 64
columns, so that small and medium rows of the product sum several terms per entry too) | "clustered" (280-320
columns inside three adjacent column ranges of 2^lg_range columns; the rows of one family share the three ranges, and
family 2j + 1 sits right behind family 2j).  Rows of A (by name, see ``names``): empty rows first / in the middle /
last, a row over empty B rows only, rows of exactly 1 / 64 / 65 / 512 / 513 / 1024 / 1025 products, a 512-product row whose LAST product
in expansion order has column N - 1, random small rows, medium rows, "sparse-large" rows (1100-6400 products over
spread B rows), "hub-large" rows (thousands of products in three ranges, many duplicate columns), a "cap" row (six
adjacent bins of ~300 products) and one mixed row.

``census`` restates, on the host, what the large-row path of csrc/spspmm.hip does with each large row (bins per column
range, then the merge of consecutive bins of at most 1024 products into groups that close at 1024 products or after
256 ranges), so that a test can assert that its input reaches a route BEFORE it looks at the GPU.
"""
import numpy as np

K = 4096
SMALL_CAP, MEDIUM_CAP = 512, 1024     # products per row: small <= 512 < medium <= 1024 < large
BIN_CAP, GROUP_CAP, GROUP_SPAN = 1024, 1024, 256

# layout of the rows of B
_EMPTY = (0, 256)
_TINY = (256, 512)        # 1-3 entries; the first 64 have exactly one
_SPREAD = (512, 2560)     # the first 1024 have exactly 16 entries
_CLUSTER = (2560, 3584)   # 16 families of 64 rows
_TAIL_EMPTY = (3584, K)
_N_FAMILIES, _FAMILY_ROWS = 16, 64


def _stratified(rng, lo, width, count):
    """`count` distinct sorted ids in [lo, lo + width): one per stratum."""
    step = width // count
    assert step >= 1
    return lo + np.arange(count, dtype=np.int64) * step + rng.integers(0, step, size=count)


def _build_b(rng, N, lg_range):
    nr = (N + (1 << lg_range) - 1) >> lg_range
    assert nr >= 16, 'the generator wants at least 16 column ranges'
    rows = [np.zeros(0, np.int64) for _ in range(K)]
    for r in range(*_TINY):
        n = 1 if r < _TINY[0] + 64 else int(rng.integers(1, 4))
        rows[r] = np.unique(rng.integers(0, N, size=n))
    # the first 512 spread rows draw each of their 16 columns from 4 candidates per stratum, so that the products of a
    # row over several of them repeat columns (sums of several terms in the small and medium rows too)
    step16 = N // 16
    pool = np.arange(16, dtype=np.int64)[:, None] * step16 + rng.integers(0, step16, size=(16, 4))
    for r in range(*_SPREAD):
        n = 16 if r < _SPREAD[0] + 1024 else int(rng.integers(12, 21))
        if r < _SPREAD[0] + 512:
            rows[r] = pool[np.arange(16), rng.integers(0, 4, size=16)]
        else:
            rows[r] = _stratified(rng, 0, N, n)
    # the last exactly-16 spread row ends on the last valid column id
    last16 = _SPREAD[0] + 1023
    rows[last16][-1] = N - 1
    bases = np.zeros(_N_FAMILIES, np.int64)
    for j in range(_N_FAMILIES // 2):
        bases[2 * j] = int(rng.integers(0, nr - 7))  # both families stay clear of the (possibly partial) last range
        bases[2 * j + 1] = bases[2 * j] + 3
    for r in range(*_CLUSTER):
        f = (r - _CLUSTER[0]) // _FAMILY_ROWS
        rows[r] = _stratified(rng, int(bases[f]) << lg_range, 3 << lg_range, int(rng.integers(280, 321)))
    return rows, bases


def _pick(rng, lo, hi, count):
    return np.sort(rng.choice(np.arange(lo, hi), size=count, replace=False))


def make_case(N, lg_range, seed=0, large='all'):
    """large: 'all' | 'one' (a single hub row) | 'none' (no row of more than 1024 products)."""
    assert large in ('all', 'one', 'none')
    rng = np.random.default_rng([seed, N & 0xFFFFFFFF, N >> 32, lg_range])
    b_rows, bases = _build_b(rng, N, lg_range)
    len_b = np.array([r.size for r in b_rows], np.int64)
    s16 = _SPREAD[0]                 # exactly-16 rows: [s16, s16 + 1024)
    one = _TINY[0]                   # exactly-1 rows: [one, one + 64)
    fam = lambda f: (_CLUSTER[0] + f * _FAMILY_ROWS, _CLUSTER[0] + (f + 1) * _FAMILY_ROWS)  # noqa: E731

    a_rows, names = [], []

    def add(name, cols):
        names.append(name)
        a_rows.append(np.unique(np.asarray(cols, np.int64)))

    def exact(p):
        cols = list(_pick(rng, s16, s16 + 1023, p // 16))
        if p % 16:
            assert p % 16 == 1
            cols.append(int(rng.integers(one, one + 64)))
        return cols

    add('empty_first', [])
    add('empty_first', [])
    add('only_empty_b', _pick(rng, *_EMPTY, 20))
    for p in (1, 64, 65, 512, 513, 1024, 1025):
        if p > MEDIUM_CAP and large != 'all':
            continue
        add('exact_%d' % p, exact(p))
    # 512 products, the last one (last A entry = highest B row, last entry of that row) on column N - 1
    add('sentinel_512', list(_pick(rng, s16, s16 + 1023, 31)) + [s16 + 1023])
    for _ in range(12):
        add('small', _pick(rng, 0, _SPREAD[1], int(rng.integers(1, 21))))
    add('empty_middle', [])
    add('empty_middle', [])
    for _ in range(3):
        add('medium', _pick(rng, s16, s16 + 1024, int(rng.integers(33, 65))))
    if large == 'all':
        for cnt in (69, 120, 200, 260, 330, 400):  # 1104 .. 6400 products over exactly-16 rows
            add('sparse_large', _pick(rng, s16, s16 + 1024, cnt))
        add('sparse_large', _pick(rng, s16 + 1024, _SPREAD[1], 150))  # rows of 12-20 entries
        for f in (0, 2, 5, 7):
            add('hub_large', _pick(rng, *fam(f), int(rng.integers(30, 61))))
        add('cap_large', list(_pick(rng, *fam(0), 3)) + list(_pick(rng, *fam(1), 3)))
        add('mixed_large', list(_pick(rng, *_EMPTY, 5)) + [one + 3] + list(_pick(rng, *_SPREAD, 20)) +
            list(_pick(rng, *fam(4), 10)) + list(_pick(rng, *_TAIL_EMPTY, 3)))
    elif large == 'one':
        add('hub_large', _pick(rng, *fam(0), 40))
    add('empty_last', [])
    add('empty_last', [])

    m = len(a_rows)
    rowptrA = np.zeros(m + 1, np.int64)
    rowptrA[1:] = np.cumsum([r.size for r in a_rows])
    colA = np.concatenate(a_rows) if m else np.zeros(0, np.int64)
    rowptrB = np.zeros(K + 1, np.int64)
    rowptrB[1:] = np.cumsum(len_b)
    colB = np.concatenate(b_rows)
    assert colB.min() >= 0 and colB.max() == N - 1
    for r in b_rows:
        assert r.size < 2 or bool((np.diff(r) > 0).all())
    rowA = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptrA))
    rowB = np.repeat(np.arange(K, dtype=np.int64), len_b)
    case = dict(N=N, lg_range=lg_range, seed=seed, m=m, k=K, names=names, rowptrA=rowptrA, colA=colA, rowA=rowA,
                rowptrB=rowptrB, colB=colB, rowB=rowB)
    case['census'] = census(case)
    return case


def row_products(case, i):
    """Columns of the products of row i of A, in expansion order (A entry order, then B entry order)."""
    rpA, rpB = case['rowptrA'], case['rowptrB']
    parts = [case['colB'][rpB[c]:rpB[c + 1]] for c in case['colA'][rpA[i]:rpA[i + 1]]]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def classify_bins(bins):
    """What spspmm_large_classify_kernel does with the per-range bin sizes of one large row:
    -> (big bins, groups closed by the 1024-product cap, groups closed by the 256-range span, groups in all)."""
    big = by_cap = by_span = groups = 0
    cur, first = 0, -1
    for q in np.nonzero(bins)[0]:
        n = int(bins[q])
        # (the empty bins between two non-empty ones only advance the span: once it reaches 256 the group is closed,
        # at the latest in front of this bin)
        if cur > 0 and q - first >= GROUP_SPAN:
            by_span += 1
            groups += 1
            cur = 0
        if n > BIN_CAP:
            if cur > 0:
                groups += 1
            cur = 0
            big += 1
            continue
        if cur > 0 and cur + n > GROUP_CAP:
            by_cap += 1
            groups += 1
            cur = 0
        if cur == 0:
            first = q
        cur += n
    if cur > 0:
        groups += 1
    return big, by_cap, by_span, groups


def census(case):
    rpA, rpB, lg = case['rowptrA'], case['rowptrB'], case['lg_range']
    len_b = np.diff(rpB)
    m = case['m']
    prod = np.array([int(len_b[case['colA'][rpA[i]:rpA[i + 1]]].sum()) for i in range(m)], np.int64)
    nr = (case['N'] + (1 << lg) - 1) >> lg
    large = {}
    for i in np.nonzero(prod > MEDIUM_CAP)[0]:
        cols = row_products(case, i)
        q, cnt = np.unique(cols >> lg, return_counts=True)
        bins = np.zeros(nr, np.int64)
        bins[q] = cnt
        big, by_cap, by_span, groups = classify_bins(bins)
        # largest number of products inside any window of 256 consecutive ranges
        cs = np.concatenate([[0], np.cumsum(bins)])
        w = min(GROUP_SPAN, nr)
        window_max = int((cs[w:] - cs[:-w]).max())
        large[int(i)] = dict(name=case['names'][i], products=int(prod[i]), max_bin=int(cnt.max()), big_bins=big,
                             closed_by_cap=by_cap, closed_by_span=by_span, groups=groups,
                             extent=int(q[-1] - q[0] + 1), window_max=window_max)
    return dict(products=prod, n_empty=int((prod == 0).sum()), n_small=int(((prod > 0) & (prod <= SMALL_CAP)).sum()),
                n_medium=int(((prod > SMALL_CAP) & (prod <= MEDIUM_CAP)).sum()), n_large=len(large), large=large)


def assert_reaches_every_route(case):
    """The census conditions of a full case (large='all'): hard asserts, never skips."""
    c = case['census']
    prod, names = c['products'], case['names']
    assert c['n_small'] >= 1 and c['n_medium'] >= 1 and c['n_large'] >= 1 and c['n_empty'] >= 6
    for p in (1, 64, 65, 512, 513, 1024, 1025):
        assert prod[names.index('exact_%d' % p)] == p
    s = names.index('sentinel_512')
    assert prod[s] == 512 and row_products(case, s)[-1] == case['N'] - 1
    assert prod[names.index('only_empty_b')] == 0 and case['rowptrA'][names.index('only_empty_b') + 1] > \
        case['rowptrA'][names.index('only_empty_b')]
    assert prod[0] == 0 and prod[-1] == 0
    L = c['large'].values()
    assert any(r['max_bin'] > BIN_CAP for r in L), 'no (row, range) bin above 1024 products'
    assert any(r['name'] == 'hub_large' and r['max_bin'] > 2 * BIN_CAP for r in L)
    # a row whose groups can ONLY close by span: bins more than 256 ranges apart, no 256-range window with 1024 products
    assert any(r['closed_by_span'] > 0 and r['closed_by_cap'] == 0 and r['big_bins'] == 0 and
               r['extent'] > GROUP_SPAN and r['window_max'] < GROUP_CAP for r in L), 'no group closed by span alone'
    assert any(r['closed_by_cap'] > 0 for r in L), 'no group closed by the 1024-product cap'
    assert all(1100 <= r['products'] <= 6400 for r in L if r['name'] == 'sparse_large')


def values(case, kind, seed=0):
    """(valA, valB) as float64.  'dyadic': half-integers in [-2, 2] (every sum exact in fp32, any order gives the same
    bits); 'uniform': uniform in (-0.5, 0.5) (rounding-sensitive)."""
    rng = np.random.default_rng([seed, 77, case['N'] & 0xFFFFFFFF])
    na, nb = case['colA'].size, case['colB'].size
    if kind == 'dyadic':
        return rng.integers(-4, 5, size=na) / 2.0, rng.integers(-4, 5, size=nb) / 2.0
    assert kind == 'uniform'
    va, vb = rng.random(na) - 0.5, rng.random(nb) - 0.5
    va[va == -0.5] = 0.25
    vb[vb == -0.5] = 0.25
    return va, vb
