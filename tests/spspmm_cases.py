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
256 ranges), so that a test can assert that its input reaches a route BEFORE it looks at the GPU; per large row it also
lists the products of every group and of every big bin.

``make_case`` needs at least 16 column ranges.  ``make_narrow_case`` (further down) builds the products of 1..15 ranges --
N from 1 column on -- with a named row of A for every edge the kernels have there; ``grid_case`` picks the generator.
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
    -> (big bins, groups closed by the 1024-product cap, groups closed by the 256-range span, groups in all,
        products of every group in list order, products of every big bin in list order)."""
    big = by_cap = by_span = 0
    group_sizes, big_sizes = [], []
    cur, first = 0, -1
    for q in np.nonzero(bins)[0]:
        n = int(bins[q])
        # (the empty bins between two non-empty ones only advance the span: once it reaches 256 the group is closed,
        # at the latest in front of this bin)
        if cur > 0 and q - first >= GROUP_SPAN:
            by_span += 1
            group_sizes.append(cur)
            cur = 0
        if n > BIN_CAP:
            if cur > 0:
                group_sizes.append(cur)
            cur = 0
            big += 1
            big_sizes.append(n)
            continue
        if cur > 0 and cur + n > GROUP_CAP:
            by_cap += 1
            group_sizes.append(cur)
            cur = 0
        if cur == 0:
            first = q
        cur += n
    if cur > 0:
        group_sizes.append(cur)
    return big, by_cap, by_span, len(group_sizes), group_sizes, big_sizes


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
        big, by_cap, by_span, groups, group_sizes, big_sizes = classify_bins(bins)
        # largest number of products inside any window of 256 consecutive ranges
        cs = np.concatenate([[0], np.cumsum(bins)])
        w = min(GROUP_SPAN, nr)
        window_max = int((cs[w:] - cs[:-w]).max())
        large[int(i)] = dict(name=case['names'][i], products=int(prod[i]), max_bin=int(cnt.max()), big_bins=big,
                             closed_by_cap=by_cap, closed_by_span=by_span, groups=groups, group_sizes=group_sizes,
                             big_sizes=big_sizes, bins=bins, extent=int(q[-1] - q[0] + 1), window_max=window_max)
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
    nr = (case['N'] + (1 << case['lg_range']) - 1) >> case['lg_range']
    if nr > GROUP_SPAN:
        # a row whose groups can ONLY close by span: bins more than 256 ranges apart, no 256-range window with 1024
        # products
        assert any(r['closed_by_span'] > 0 and r['closed_by_cap'] == 0 and r['big_bins'] == 0 and
                   r['extent'] > GROUP_SPAN and r['window_max'] < GROUP_CAP for r in L), 'no group closed by span alone'
    else:  # a group spans at most nr ranges: with at most 256 of them none can close by span
        assert all(r['closed_by_span'] == 0 for r in L), 'a group closed by span with at most 256 ranges'
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


# ----------------------------------------------------------------------------------------------------------------------
# Ordinary widths: 1 <= nr <= 15 column ranges (make_case needs 16).  B is built by row kinds (blocks), every row of A
# has a name, and the census below asserts what each named row is for -- see docs/design/spspmm.md, "Ordinary widths".
# ----------------------------------------------------------------------------------------------------------------------
EXACT_P = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)  # class edges and the keys-per-lane ladder
GROUP_G = (64, 65, 128, 129, 256, 257, 512, 513, 1024)           # the same ladder for the one-wave path of the groups
COUNT_LANES, COUNT_LONG = 8, 512   # spspmm_count_kernel: lanes per row of A, entries beyond which the wave takes a row


def make_narrow_case(N, lg_range, seed=0):
    """A (m x k) * B (k x N) for 1 <= ceil(N / 2^lg_range) <= 15.  Blocks of B (rows by kind):
      empty | last: 3072 rows {N - 1} | distinct: 1024 one-entry rows (all-distinct columns when N >= 1024) |
      stride: 512 one-entry rows, column j * 2^s (N >= 2^lg_range) | wide: 1100 rows of min(16, N) columns, half of
      them from a pool of 256 columns | single: 64 random one-entry rows | low / runcol / high: one-entry rows below, on
      and above column N // 2 | cover0 / cover_tail: 64-column pieces that tile range 0 / the last, partial range |
      cancel_*: pairs of rows with identical columns | long_b: one row of min(N, 3000) columns | r0rows / r1rows:
      16-column rows inside range 0 / 1 | lastrange: 1024 one-entry rows inside the last range."""
    R = 1 << lg_range
    nr = (N + R - 1) >> lg_range
    assert N >= 1 and 1 <= nr <= 15, 'make_narrow_case is for 1..15 column ranges (make_case takes 16 and more)'
    rng = np.random.default_rng([seed, N, lg_range, 0x6e6172])
    last_lo = (nr - 1) * R        # the last range: [last_lo, N)
    last_w = N - last_lo
    r0_w = min(R, N)              # range 0: [0, r0_w)
    w = min(16, N)
    c_run = N // 2
    one = lambda c: np.array([c], np.int64)  # noqa: E731

    b_rows, blk = [], {}

    def block(name, rows):
        blk[name] = (len(b_rows), len(b_rows) + len(rows))
        b_rows.extend(np.asarray(r, np.int64) for r in rows)

    def tiles(lo, hi):
        return [np.arange(s, min(s + 64, hi), dtype=np.int64) for s in range(lo, hi, 64)]

    block('empty', [np.zeros(0, np.int64)] * 64)
    block('last', [one(N - 1)] * 3072)
    block('distinct', [one(j * N // 1024 if N >= 1024 else j % N) for j in range(1024)])
    stride = 0
    if N >= R:
        stride = 1 << ((N // 512).bit_length() - 1)
        block('stride', [one(j * stride) for j in range(512)])
    pool = np.sort(rng.choice(N, size=min(N, 256), replace=False))
    wide = [pool[_stratified(rng, 0, pool.size, min(w, pool.size))] for _ in range(550)]
    wide += [_stratified(rng, 0, N, w) for _ in range(550)]
    block('wide', wide)
    block('single', [one(int(rng.integers(0, N))) for _ in range(64)])
    if N >= 2:
        block('low', [one(j % c_run) for j in range(256)])
        block('runcol', [one(c_run)] * 16)
    if N >= 3:
        block('high', [one(c_run + 1 + j % (N - 1 - c_run)) for j in range(300)])
    block('cover0', tiles(0, r0_w))
    if N % R not in (0, 1):
        block('cover_tail', tiles(last_lo, N))
    pair = lambda cols: [cols, cols.copy()]  # noqa: E731
    block('cancel_small', pair(_stratified(rng, 0, N, min(N, 100))))
    if N >= 257:
        block('cancel_medium', pair(_stratified(rng, 0, N, min(N, 400))))
    if r0_w >= 600:
        block('cancel_big_bin', pair(_stratified(rng, 0, r0_w, 600)))
    if nr >= 2:  # 512 columns of range 0 (a bin of exactly 1024 products) and up to 200 of the last range
        block('cancel_group', pair(np.concatenate([_stratified(rng, 0, R, 512),
                                                   _stratified(rng, last_lo, last_w, min(last_w, 200))])))
    if N >= 1025:
        block('long_b', [_stratified(rng, 0, N, min(N, 3000))])
    if nr >= 2:
        block('r0rows', [_stratified(rng, 0, R, 16) for _ in range(70)])
        block('lastrange', [one(last_lo + int(rng.integers(0, last_w))) for _ in range(1024)])
    if nr >= 3:
        block('r1rows', [_stratified(rng, R, R, 16) for _ in range(38)])
    k = len(b_rows)

    a_rows, names, cancel = [], [], []
    rows_of = lambda name, lo=0, hi=None: np.arange(blk[name][0] + lo, blk[name][0] + hi if hi is not None  # noqa: E731
                                                    else blk[name][1])

    def add(name, *parts):
        names.append(name)
        cols = np.concatenate([np.asarray(p, np.int64).ravel() for p in parts]) if parts else np.zeros(0, np.int64)
        a_rows.append(np.unique(cols))
        assert a_rows[-1].size == cols.size, name  # no part names a row of B twice

    def exact(p):
        return [_pick(rng, *blk['wide'], p // w)] + ([_pick(rng, *blk['single'], p % w)] if p % w else [])

    add('empty_first')
    add('empty_first')
    add('only_empty_b', _pick(rng, *blk['empty'], 20))
    for p in EXACT_P:
        add('exact_%d' % p, *exact(p))
    if N >= 2:  # (with one column every run starts at position 0)
        hi20 = [rows_of('high', 0, 20)] if N >= 3 else []
        add('run_cross_64', rows_of('low', 0, 60), rows_of('runcol', 0, 11), *hi20)    # the run: positions 60..70
        add('run_from_63', rows_of('low', 0, 63), rows_of('runcol', 0, 10), *hi20)     # head in lane 63
    if N >= 3:  # (a medium row needs products behind the run as well: three columns)
        add('run_cross_256', rows_of('low', 0, 250), rows_of('runcol', 0, 13), rows_of('high'))  # positions 250..262
        add('run_from_255', rows_of('low', 0, 255), rows_of('runcol', 0, 10), rows_of('high'))
    add('one_column_512', rows_of('last', 0, 512))
    add('one_column_1024', rows_of('last', 0, 1024))
    add('one_column_large', rows_of('last', 0, 3000))
    if N >= 512:
        add('distinct_512', rows_of('distinct', 0, 1024)[::2] if N >= 1024 else rows_of('distinct', 0, 512))
    if N >= 1024:
        add('distinct_1024', rows_of('distinct'))
    if N >= R:
        add('stride_512', rows_of('stride'))
    for _ in range(12):
        add('small', _pick(rng, blk['wide'][0], blk['single'][1], int(rng.integers(1, 21))))
    add('empty_middle')
    add('empty_middle')
    for _ in range(3):
        add('medium', _pick(rng, *blk['wide'], int(rng.integers(-(-513 // w), 1024 // w + 1))))
    # range 0 in full (plus a few rows anywhere); padded to a large row where range 0 has few columns
    n_cover = sum(b_rows[r].size for r in rows_of('cover0'))
    pad = [rows_of('wide', 0, -(-(1030 - n_cover) // w))] if n_cover <= MEDIUM_CAP else []
    add('dense_range', rows_of('cover0'), rows_of('wide', 1090, 1100), *pad)
    if 'cover_tail' in blk:
        n_cover = sum(b_rows[r].size for r in rows_of('cover_tail'))
        add('dense_tail', rows_of('cover_tail'), rows_of('wide', 1080, 1090),
            *([rows_of('last', 0, 1100)] if n_cover <= MEDIUM_CAP else []))
    if N % R == 1 and nr >= 2:
        add('tail_one', rows_of('cover0'), rows_of('last', 0, 700))
    for name in ('cancel_small', 'cancel_medium', 'cancel_big_bin', 'cancel_group'):
        if name in blk:
            add(name, rows_of(name))
            cancel.append((name, len(a_rows) - 1, blk[name][0], blk[name][0] + 1))
    # the count kernel gives 8 lanes to a row of A: rows 8j .. 8j + 7 share a wave.  Three rows of more than 512 entries
    # inside one wave (its `todo` loop), right behind the last row the 8 lanes still take themselves
    while len(a_rows) % COUNT_LANES > COUNT_LANES - 4:
        add('small', _pick(rng, *blk['wide'], 2))
    add('long_a_512', rows_of('distinct', 0, 512))
    add('long_a_513', rows_of('distinct', 0, 513))
    add('long_a_2000', rows_of('distinct'), rows_of('last', 0, 976))
    add('long_a_third', rows_of('last', 100, 700))
    if 'long_b' in blk:
        add('one_long_b', rows_of('long_b'))
    if nr >= 2:
        for g in GROUP_G:  # a bin above 1024 products in range 0, a group of exactly g products in the last range
            add('group_%d' % g, rows_of('r0rows'), rows_of('lastrange', 0, g))
    if nr >= 3:  # big bin | 608 products | 600 products: the first group closes by the cap, the second stays open
        add('mixed_bins', rows_of('r0rows'), rows_of('r1rows'), rows_of('lastrange', 0, 600))
    add('empty_last')
    add('empty_last')

    m = len(a_rows)
    len_b = np.array([r.size for r in b_rows], np.int64)
    rowptrA = np.zeros(m + 1, np.int64)
    rowptrA[1:] = np.cumsum([r.size for r in a_rows])
    colA = np.concatenate(a_rows)
    rowptrB = np.zeros(k + 1, np.int64)
    rowptrB[1:] = np.cumsum(len_b)
    colB = np.concatenate(b_rows)
    assert colB.min() >= 0 and colB.max() == N - 1
    for r in b_rows:
        assert r.size < 2 or bool((np.diff(r) > 0).all())
    rowA = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowptrA))
    rowB = np.repeat(np.arange(k, dtype=np.int64), len_b)
    case = dict(N=N, lg_range=lg_range, seed=seed, m=m, k=k, names=names, rowptrA=rowptrA, colA=colA, rowA=rowA,
                rowptrB=rowptrB, colB=colB, rowB=rowB, blocks=blk, cancel=cancel, run_col=c_run, stride=stride)
    case['census'] = census(case)
    return case


def run_positions(case, i, col):
    """First and last position of column `col` in the sorted products of row i, and how many there are."""
    pos = np.nonzero(np.sort(row_products(case, i), kind='stable') == col)[0]
    return int(pos[0]), int(pos[-1]), int(pos.size)


def row_class(p):
    return 'empty' if p == 0 else 'small' if p <= SMALL_CAP else 'medium' if p <= MEDIUM_CAP else 'large'


def assert_reaches_narrow_routes(case):
    """The census conditions of a narrow case: hard asserts, never skips.  A named row is absent only where N makes it
    impossible, and that is asserted too."""
    c, names, N, lg = case['census'], case['names'], case['N'], case['lg_range']
    prod, large = c['products'], c['large']
    R = 1 << lg
    nr = (N + R - 1) >> lg
    last_lo = (nr - 1) * R
    idx = names.index
    entries = np.diff(case['rowptrA'])
    len_b = np.diff(case['rowptrB'])
    cls = lambda name: row_class(int(prod[idx(name)]))  # noqa: E731
    assert 1 <= nr <= 15 and int(case['colB'].max()) == N - 1
    assert c['n_small'] >= 1 and c['n_medium'] >= 1 and c['n_large'] >= 1 and c['n_empty'] >= 7

    # empty rows first, in the middle and last; a row over empty rows of B
    assert names[0] == names[1] == 'empty_first' and names[-1] == names[-2] == 'empty_last'
    assert prod[0] == 0 and prod[-1] == 0 and entries[0] == 0 and entries[-1] == 0
    i = idx('empty_middle')
    assert 2 < i < case['m'] - 3 and entries[i] == 0 and entries[i - 1] > 0
    assert prod[idx('only_empty_b')] == 0 and entries[idx('only_empty_b')] == 20

    for p in EXACT_P:
        assert prod[idx('exact_%d' % p)] == p

    # runs of one column across the 64- and 256-entry chunks of compress_and_store
    for name, first, last, klass, need in (('run_cross_64', 60, 70, 'small', 2), ('run_from_63', 63, 72, 'small', 2),
                                           ('run_cross_256', 250, 262, 'medium', 3),
                                           ('run_from_255', 255, 264, 'medium', 3)):
        assert (name in names) == (N >= need), name
        if name in names:
            assert run_positions(case, idx(name), case['run_col']) == (first, last, last - first + 1), name
            assert cls(name) == klass, name

    for name, p in (('one_column_512', 512), ('one_column_1024', 1024), ('one_column_large', 3000)):
        cols = row_products(case, idx(name))
        assert cols.size == p and bool((cols == N - 1).all()), name
    assert (cls('one_column_512'), cls('one_column_1024'), cls('one_column_large')) == ('small', 'medium', 'large')

    # hash sets of the symbolic stage at full load: 512 distinct columns in 1024 slots, 1024 in 2048
    for name, p, need in (('distinct_512', 512, 512), ('distinct_1024', 1024, 1024), ('stride_512', 512, R)):
        assert (name in names) == (N >= need), name
        if name in names:
            cols = row_products(case, idx(name))
            assert cols.size == p and np.unique(cols).size == p, name
    if 'stride_512' in names:
        s = case['stride']
        assert s == 1 << (s.bit_length() - 1) and s * 1024 > N >= s * 512
        assert np.array_equal(np.sort(row_products(case, idx('stride_512'))), np.arange(512) * s)

    # dense rows of C: every column of range 0, every column of a partial last range
    r0_w = min(R, N)
    cols = np.unique(row_products(case, idx('dense_range')))
    assert cls('dense_range') == 'large' and np.array_equal(cols[cols < R], np.arange(r0_w))
    assert large[idx('dense_range')]['bins'][0] > BIN_CAP
    assert ('dense_tail' in names) == (N % R not in (0, 1))
    if 'dense_tail' in names:
        cols = np.unique(row_products(case, idx('dense_tail')))
        assert cls('dense_tail') == 'large' and np.array_equal(cols[cols >= last_lo], np.arange(last_lo, N))
        assert large[idx('dense_tail')]['bins'][nr - 1] > BIN_CAP
    assert ('tail_one' in names) == (N % R == 1 and nr >= 2)  # (N = 1: the single column IS range 0)
    if 'tail_one' in names:
        bins = large[idx('tail_one')]['bins']
        assert N - last_lo == 1 and bins[0] > BIN_CAP and 1 <= bins[nr - 1] <= BIN_CAP
        assert large[idx('tail_one')]['big_bins'] == 1 and large[idx('tail_one')]['groups'] >= 1

    # cancelling rows: two entries of A over two rows of B with identical columns
    for name, need, klass in (('cancel_small', True, 'small'), ('cancel_medium', N >= 257, 'medium'),
                              ('cancel_big_bin', r0_w >= 600, 'large'), ('cancel_group', nr >= 2, 'large')):
        assert (name in names) == bool(need), name
        assert (name in names) == (name in [t[0] for t in case['cancel']])
    for name, i, b1, b2 in case['cancel']:
        assert idx(name) == i and entries[i] == 2
        assert list(case['colA'][case['rowptrA'][i]:case['rowptrA'][i + 1]]) == [b1, b2]
        rp = case['rowptrB']
        assert np.array_equal(case['colB'][rp[b1]:rp[b1 + 1]], case['colB'][rp[b2]:rp[b2 + 1]]) and len_b[b1] > 0
        assert int((case['colA'] == b1).sum()) == 1 and int((case['colA'] == b2).sum()) == 1  # nobody else reads them
    if 'cancel_big_bin' in names:
        r = large[idx('cancel_big_bin')]
        assert r['big_bins'] == 1 and r['groups'] == 0
    if 'cancel_group' in names:
        r = large[idx('cancel_group')]
        assert r['big_bins'] == 0 and r['groups'] >= 1 and r['group_sizes'][0] == GROUP_CAP and r['closed_by_cap'] >= 1

    # spspmm_count_kernel: 512 entries (eight lanes), 513 (the whole wave), three long rows inside one wave
    for name, n in (('long_a_512', 512), ('long_a_513', 513), ('long_a_2000', 2000)):
        i = idx(name)
        assert entries[i] == n == prod[i], name
        assert bool((len_b[case['colA'][case['rowptrA'][i]:case['rowptrA'][i + 1]]] == 1).all()), name
    trio = [idx('long_a_513'), idx('long_a_2000'), idx('long_a_third')]
    assert trio == list(range(trio[0], trio[0] + 3)) and len({i // COUNT_LANES for i in trio}) == 1
    assert all(entries[i] > COUNT_LONG for i in trio) and entries[idx('long_a_512')] == COUNT_LONG
    assert idx('long_a_512') // COUNT_LANES == trio[0] // COUNT_LANES  # the eight-lane path beside them

    assert ('one_long_b' in names) == (N >= 1025)
    if 'one_long_b' in names:
        i = idx('one_long_b')
        assert entries[i] == 1 and prod[i] == min(N, 3000) and cls('one_long_b') == 'large'

    L = list(large.values())
    assert all(r['closed_by_span'] == 0 for r in L)  # a group spans at most nr <= 15 ranges
    if nr == 1:  # a large row is ONE bin of more than 1024 products: the small-bin list is empty
        assert len(L) >= 1 and all(r['big_bins'] == 1 and r['groups'] == 0 for r in L)
        assert any(r['big_sizes'] == [MEDIUM_CAP + 1] for r in L)  # the smallest big bin there is
        assert not any(n.startswith('group_') or n == 'mixed_bins' for n in names)
    else:
        assert any(r['big_bins'] >= 1 and r['groups'] >= 1 for r in L), 'no big bin beside a group'
        assert any(r['closed_by_cap'] >= 1 for r in L), 'no group closed by the 1024-product cap'
        assert any(r['groups'] > r['closed_by_cap'] for r in L), 'no group left open at the end of its row'
        for g in GROUP_G:
            r = large[idx('group_%d' % g)]
            assert r['big_bins'] == 1 and r['group_sizes'] == [g], g
        assert ('mixed_bins' in names) == (nr >= 3)
        if nr >= 3:  # all three in ONE row
            r = large[idx('mixed_bins')]
            assert r['big_bins'] == 1 and r['closed_by_cap'] == 1 and r['groups'] == 2

    assert sum(n == 'small' for n in names) >= 12 and sum(n == 'medium' for n in names) == 3
    assert all(row_class(int(prod[i])) == n for i, n in enumerate(names) if n in ('small', 'medium'))


# ---- the grid of tests/test_spspmm_narrow_gpu.py: N in units of the range width R = 2^lg_range (8192 fp32, 4096 fp64) ----
def narrow_grid(lg_range):
    R = 1 << lg_range
    return [1, 2, 97, R, R + 1, 2 * R, 2 * R + 1, 8 * R, 15 * R - 3]


def ordinary_grid(lg_range):
    """The narrow widths, then the widths make_case builds (16 ranges and more) up to 2^22 columns."""
    return narrow_grid(lg_range) + [16 << lg_range, 500000, 1 << 21, 1 << 22]


_GRID_CASES = {}


def grid_case(N, lg_range):
    """The case of one grid point, built once per process (read-only by convention): make_narrow_case below 16 ranges,
    seeded by its place in the grid, make_case from there on."""
    key = (N, lg_range)
    if key not in _GRID_CASES:
        grid = ordinary_grid(lg_range)
        nr = (N + (1 << lg_range) - 1) >> lg_range
        _GRID_CASES[key] = make_narrow_case(N, lg_range, seed=1 + grid.index(N)) if nr < 16 else \
            make_case(N, lg_range, seed=0)
    return _GRID_CASES[key]


def assert_census(case):
    nr = (case['N'] + (1 << case['lg_range']) - 1) >> case['lg_range']
    (assert_reaches_narrow_routes if nr < 16 else assert_reaches_every_route)(case)
