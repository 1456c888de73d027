"""numpy oracles, censuses and the shared case lists for the index kernels: the exclusive scan (csrc/scan.hip),
ind2ptr / ptr2ind (csrc/convert.hip, csrc/expand.h) and select / filter / scatter_rows / diag (csrc/select.hip).

Plain numpy, no torch.  Everything is int64 (masks: uint8) and every comparison made with it is bit-exact.

  * oracles: one per entry point, written from the contract in include/tsamd.h and NOT from the kernels' arithmetic
    (searchsorted / repeat / boolean indexing; the diag family is a stable sort of the concatenated entries by
    (row, col)).  tests/test_index_reference.py holds each of them to a per-element Python loop.
  * censuses: which branch every workgroup takes, from the same sizes the kernels use.  `Sizes` comes from
    tsamd_index_route (the tests read it from the library); nothing here repeats a constant of the kernels.
  * cases: the inputs of tests/test_index_kernels_gpu.py, every one with the census it is built for
    (`want`, checked by `*_target_ok`): on the CPU in tests/test_index_reference.py, and again on the GPU before
    the comparison.
"""
from collections import namedtuple

import numpy as np

Sizes = namedtuple('Sizes', 'scan_tile expand_tile filter_tile filter_slice long_run')
WAVE = 64
I64 = np.int64

PREDS = ('col_range', 'off_diag', 'mask', 'mask_row', 'mask_col', 'col_mapped')  # TSAMD_KEEP_* = the position


def sizes_from_route(words):
    """the eight words of tsamd_index_route -> Sizes"""
    assert len(words) == 8 and all(int(w) == 0 for w in words[5:])
    return Sizes(*(int(w) for w in words[:5]))


def i64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=I64))


def ceil_div(a, b):
    return -(-a // b)


def align_up(a, b):
    return ceil_div(a, b) * b


# ---------------------------------------------------------------------------------------------------------------
# scan
# ---------------------------------------------------------------------------------------------------------------
def exclusive_scan(x):
    """-> (out, total): out[i] = sum of x[:i], total = sum of x (int64, wrapping like the device)"""
    x = i64(x)
    out = np.zeros(x.size, I64)
    if x.size:
        np.cumsum(x[:-1], out=out[1:])
    return out, int(x.sum(dtype=I64)) if x.size else 0


def scan_census(n, sz):
    """tiles per level, top level first: [] for n <= 0, [1] for one tile, [nb, ...] above."""
    if n <= 0:
        return []
    if n <= sz.scan_tile:
        return [1]
    nb = ceil_div(n, sz.scan_tile)
    return [nb] + scan_census(nb, sz)


def scan_workspace_bytes(n, sz):
    """what the scan really uses (one 256-byte aligned array of tile sums per level above the last) + 256"""
    census = scan_census(n, sz)
    return sum(align_up(8 * nb, 256) for nb in census[:-1]) + 256


def scan_values(n, kind, seed=0):
    """'big': the running sum passes 2^32 after the first element and 2^40 at the middle one, a few negatives;
    'first' / 'last': zero except that element; 'ones'."""
    if kind == 'ones':
        return np.ones(n, I64)
    x = np.zeros(n, I64)
    if n == 0:
        return x
    if kind == 'first':
        x[0] = (1 << 40) + 3
    elif kind == 'last':
        x[-1] = (1 << 40) + 3
    else:
        assert kind == 'big'
        x = np.random.default_rng(seed).integers(-3, 1 << 20, n).astype(I64)
        x[0] += (1 << 32) + 5
        x[n // 2] += 1 << 40
    return x


def scan_cases(sz):
    """(id, n, levels the case is built for)"""
    T = sz.scan_tile
    out = []
    for n in (0, 1, 7, 8, 9, 255 * 8, T - 1, T, T + 1, 2 * T, 2 * T + 1, T * T - 1, T * T, T * T + 1):
        levels = 0 if n == 0 else 1 if n <= T else 2 if n <= T * T else 3
        out.append(('n%d-levels%d' % (n, levels), n, levels))
    return out


# ---------------------------------------------------------------------------------------------------------------
# ind2ptr / ptr2ind
# ---------------------------------------------------------------------------------------------------------------
def ind2ptr(ind, M):
    """ptr[i] = number of entries with id < i, i in [0, M]"""
    return np.searchsorted(i64(ind), np.arange(M + 1, dtype=I64), side='left').astype(I64)


def ptr2ind(ptr):
    ptr = i64(ptr)
    return np.repeat(np.arange(ptr.size - 1, dtype=I64), np.diff(ptr))


def ind2ptr_census(ind, M, sz):
    """per boundary t in [0, E]: (lo, hi, pointers the boundary owns, 'inline' | 'long').  E = 0 is a memset: []"""
    ind = i64(ind)
    E = ind.size
    if E == 0:
        return []
    lo = np.concatenate(([0], ind + 1))
    hi = np.concatenate((ind, [M]))
    lo, hi = np.maximum(lo, 0), np.minimum(hi, M)
    return [(int(a), int(b), int(b - a + 1), 'long' if b - a >= sz.long_run else 'inline') for a, b in zip(lo, hi)]


def expand_census(ptr, nseg, total, sz):
    """ptr2ind (ptr = rowptr, nseg = M) and select_fill (ptr = out_ptr, nseg = K): per tile of kExpandTile entries
    (lo, hi, segments it intersects, 'staged' | 'search').  The first / last segment is the LAST one whose pointer is
    <= the tile's first / last entry, among ptr[0 .. nseg)."""
    p = i64(ptr)[:nseg]
    out = []
    for e0 in range(0, total, sz.expand_tile):
        e1 = min(e0 + sz.expand_tile, total)
        lo = int(np.searchsorted(p, e0, side='right')) - 1
        hi = int(np.searchsorted(p, e1 - 1, side='right')) - 1
        n = hi - lo + 1
        out.append((lo, hi, n, 'staged' if n <= sz.expand_tile else 'search'))
    return out


def _dense(a, b):
    """one entry in every row of [a, b)"""
    return np.arange(a, b, dtype=I64)


def ind2ptr_cases(sz):
    """(id, M, ind, want): want = dict(long=<sorted pointer runs that take the long kernel>, inline=<longest inline
    run>, odd=<M + 1 odd: the pre-set stops one word short>).  Filler rows hold one entry each, so the run a case is
    named for is the only one of its kind."""
    R = sz.long_run
    rng = np.random.default_rng(11)
    out = []

    def add(name, M, ind, long, inline=None):
        ind = np.sort(i64(ind))
        want = dict(long=sorted(long), odd=(M + 1) % 2 == 1)
        if inline is not None:
            want['inline'] = inline
        out.append(('%s-M%d-E%d-%s' % (name, M, ind.size, 'long' if long else 'inline'), M, ind, want))

    # M on both sides of the long run, M + 1 even and odd; E on both sides of a block of 256 boundaries and of a tile
    sizes = (1, 255, 256, 257, sz.expand_tile - 1, sz.expand_tile, sz.expand_tile + 1)
    for j, M in enumerate((1, 2, R - 1, R, R + 1, 4 * R, 4 * R + 1)):
        for E in (sizes[j], sizes[(j + 3) % 7]):
            ind = np.sort(rng.integers(0, M, E))  # (the route in the id is whatever the draw gives)
            add('random', M, ind, [r for _, _, r, w in ind2ptr_census(ind, M, sz) if w == 'long'])
    # runs of exactly R - 2 .. R + 1 row pointers (R - 3 .. R empty rows) at the front, in the middle, at the end
    for M in (4 * R, 4 * R + 1):
        for run in (R - 2, R - 1, R, R + 1):
            long = [run] if run - 1 >= R else []
            add('front-run%d' % run, M, np.concatenate(([run - 1], _dense(run - 1, M))), long, inline=None if long else run)
            a = R + 7
            add('middle-run%d' % run, M, np.concatenate((_dense(0, a + 1), _dense(a + run, M))), long,
                inline=None if long else run)
            add('end-run%d' % run, M, _dense(0, M - run + 1), long, inline=None if long else run)
    M = 4 * R + 1
    add('all-in-row0', M, np.zeros(300, I64), [M])
    add('all-in-last-row', M, np.full(300, M - 1, I64), [M])
    add('all-in-row0', 4 * R, np.zeros(257, I64), [4 * R])
    add('all-in-last-row', 4 * R, np.full(257, 4 * R - 1, I64), [4 * R])
    return out


def ind2ptr_target_ok(census, M, want):
    long = sorted(r for _, _, r, w in census if w == 'long')
    ok = long == want['long'] and want['odd'] == ((M + 1) % 2 == 1)
    if 'inline' in want:
        ok = ok and max(r for _, _, r, w in census if w == 'inline') == want['inline']
    return ok


def ptr2ind_cases(sz):
    """(id, ptr, want): want = the (segments, route) of every tile.  The inverse of every ind2ptr case is run as well
    (test_index_kernels_gpu.py); these are the cases built for the tiles."""
    T = sz.expand_tile
    out = []

    def add(name, counts, want):
        ptr = np.concatenate(([0], np.cumsum(i64(counts)))).astype(I64)
        out.append((name, ptr, want))

    # a tile over exactly T rows (staged) and over T + 1 (search in place); the second tile holds the rest of the row
    for empty, route in ((T - 2, 'staged'), (T - 1, 'search')):
        counts = [1] + [0] * empty + [T - 1 + 10] + [0] * 3
        add('tile-over-%d-rows-%s' % (empty + 2, route), counts, [(empty + 2, route), (1, 'staged')])
    # a hub row over three tiles, small rows and empty rows around it
    add('hub-over-three-tiles-staged', [0, 0, 3, 5, 2 * T + 100, 0, 4, 1, 0], [(3, 'staged'), (1, 'staged'), (4, 'staged')])
    # E on both sides of a slice of 256 and of a tile, leading and trailing empty rows
    for E in (1, 255, 256, 257, T - 1, T, T + 1):
        counts = [0, 0] + [1] * (E // 2) + [0] + [E - E // 2] + [0, 0, 0]
        tiles = ceil_div(E, T)
        add('E%d-leading-trailing-empty-staged' % E, counts, None if tiles > 1 else [(E // 2 + (2 if E // 2 else 1), 'staged')])
    # long runs of empty rows INSIDE two tiles (a run in front of a tile's first entry is skipped by the search for
    # the last row with ptr <= e): both search in place, the third tile holds the end of the last row
    add('empty-runs-inside-two-tiles-search', [T - 1] + [0] * (T + 5) + [T] + [0] * (2 * T) + [7],
        [(T + 7, 'search'), (2 * T + 2, 'search'), (1, 'staged')])
    return out


def expand_target_ok(census, want):
    return want is None or [(n, r) for _, _, n, r in census] == [tuple(w) for w in want]


# ---------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------
def select_plan(ptr, S, idx):
    """-> (out_ptr[K + 1], total, errors): negative ids wrap; ids outside [-S, S) pick an empty segment"""
    ptr, idx = i64(ptr), i64(idx)
    j = np.where(idx < 0, idx + S, idx)
    bad = (j < 0) | (j >= S)
    js = np.where(bad, 0, j)
    cnt = np.where(bad, 0, ptr[js + 1] - ptr[js]) if idx.size and S else np.zeros(idx.size, I64)
    out_ptr = np.concatenate(([0], np.cumsum(cnt))).astype(I64)
    return out_ptr, int(out_ptr[-1]), int(bad.sum())


def select_fill(ptr, S, ind, idx):
    """-> (seg, ind_out, pos): entry e of output segment i comes from src = ptr[idx[i]] + (e - out_ptr[i])"""
    ptr, idx, ind = i64(ptr), i64(idx), i64(ind)
    out_ptr, total, _ = select_plan(ptr, S, idx)
    cnt = np.diff(out_ptr)
    seg = np.repeat(np.arange(idx.size, dtype=I64), cnt)
    j = np.where(idx < 0, idx + S, idx)
    start = np.where((j < 0) | (j >= S), 0, ptr[np.clip(j, 0, max(S - 1, 0))]) if idx.size else np.zeros(0, I64)
    cnt, start = cnt.astype(I64), start.astype(I64)
    pos = (np.repeat(start, cnt) + np.arange(total, dtype=I64) - np.repeat(out_ptr[:-1], cnt)).astype(I64)
    return seg, ind[pos], pos


def select_source(sz):
    """the pattern every select case picks from: (ptr, S, ind, ids by length).  Segments of 0, 1, 2, 3, T - 2, T - 1
    and T entries, then small random ones; the first and the last segment are not empty."""
    T = sz.expand_tile
    rng = np.random.default_rng(5)
    lens = [4, 0, 1, 2, 3, T - 2, T - 1, T] + rng.integers(0, 6, 40).tolist() + [2]
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(I64)
    ind = rng.integers(0, 1000, int(ptr[-1])).astype(I64)
    by_len = {0: 1, 1: 2, 2: 3, 3: 4, T - 2: 5, T - 1: 6, T: 7}
    return ptr, len(lens), ind, by_len


def select_cases(sz):
    """(id, idx, want): want = dict(total, errors, tiles = [(segments, route)] or None)"""
    T = sz.expand_tile
    ptr, S, _, L = select_source(sz)
    rng = np.random.default_rng(6)
    out = []

    def add(name, idx, total, errors=0, tiles=None):
        out.append((name, i64(idx), dict(total=total, errors=errors, tiles=tiles)))

    for empty, route in ((T - 2, 'staged'), (T - 1, 'search')):
        add('tile-over-%d-picks-%s' % (empty + 2, route), [L[1]] + [L[0]] * empty + [L[T - 1]] + [L[0]] * 2 + [L[3]],
            T + 3, tiles=[(empty + 2, route), (1, 'staged')])
    add('pick-straddles-tile-1-before-1-after-staged', [L[T - 1], L[2], L[3]], T + 4, tiles=[(2, 'staged'), (2, 'staged')])
    add('pick-straddles-tile-2-before-1-after-staged', [L[T - 2], L[3], L[1]], T + 2, tiles=[(2, 'staged'), (2, 'staged')])
    add('pick-straddles-tile-1-before-2-after-staged', [L[T - 1], L[3], L[0]], T + 2, tiles=[(2, 'staged'), (1, 'staged')])
    add('pick-ends-at-tile-edge-staged', [L[T], L[0], L[0], L[2]], T + 2, tiles=[(1, 'staged'), (1, 'staged')])
    add('total0-K0', [], 0, tiles=[])
    add('total0-K3-empty-picks', [L[0]] * 3, 0, tiles=[])
    add('total1-K1', [L[1]], 1, tiles=[(1, 'staged')])
    add('total%d' % (T - 1), [L[T - 1]], T - 1, tiles=[(1, 'staged')])
    add('total%d' % T, [L[T]], T, tiles=[(1, 'staged')])
    add('total%d' % (T + 1), [L[T - 1], L[2]], T + 1, tiles=[(2, 'staged'), (1, 'staged')])
    add('total%d-duplicate-ids' % (2 * T + 1), [L[T], L[T], L[1]], 2 * T + 1, tiles=[(1, 'staged'), (1, 'staged'), (1, 'staged')])
    for K in (256, 257):
        idx = rng.integers(8, S, K)  # the small segments, with duplicates
        add('K%d-duplicates' % K, idx, select_plan(ptr, S, idx)[1])
    add('ids-at-the-ends', [-S, -1, 0, S - 1, -S, S - 1], 4 + 2 + 4 + 2 + 4 + 2)
    add('invalid-ids-mixed-in', [S, L[3], -S - 1, -1, S, L[T], -S - 1, S + 100, -3 * S, 0], 3 + 2 + T + 4, errors=6)
    add('invalid-ids-only', [S, -S - 1], 0, errors=2, tiles=[])
    # long runs of empty and of invalid picks inside two tiles: both search in place
    add('empty-and-invalid-pick-runs-search', [L[T - 1]] + [L[0]] * (T + 9) + [L[T]] + [S] * (T + 1) + [L[T], L[2]],
        3 * T + 1, errors=T + 1, tiles=[(T + 11, 'search'), (T + 3, 'search'), (2, 'staged'), (1, 'staged')])
    return out


def select_target_ok(census, plan, want):
    out_ptr, total, errors = plan
    return total == want['total'] and errors == want['errors'] and expand_target_ok(census, want['tiles'])


# ---------------------------------------------------------------------------------------------------------------
# filter
# ---------------------------------------------------------------------------------------------------------------
def keep_flags(pred, row, col, mask, cmap, a, b):
    """the six predicates of include/tsamd.h -> bool[n]"""
    if pred == 'col_range':
        return (col >= a) & (col < a + b)
    if pred == 'off_diag':
        return row != col - a
    if pred == 'mask':
        return mask != 0
    if pred == 'mask_row':
        return mask[row] != 0
    if pred == 'mask_col':
        return mask[col] != 0
    if pred == 'col_mapped':
        return cmap[col] >= 0
    raise ValueError(pred)


def filter_positions(keep):
    """-> (pos[n + 1], count) of tsamd_filter_plan"""
    pos = np.concatenate(([0], np.cumsum(np.asarray(keep, bool).astype(I64)))).astype(I64)
    return pos, int(pos[-1])


def filter_compact(keep, row, col, row_map=None, col_map=None, row_shift=0, col_shift=0):
    """-> (row_out, col_out, src_out) in input order"""
    src = np.flatnonzero(np.asarray(keep, bool)).astype(I64)
    r, c = i64(row)[src], i64(col)[src]
    if row_map is not None:
        r = i64(row_map)[r]
    if col_map is not None:
        c = i64(col_map)[c]
    return (r - row_shift).astype(I64), (c - col_shift).astype(I64), src


def _classes(keep, width):
    out = []
    for s in range(0, keep.size, width):
        k = int(keep[s:s + width].sum())
        out.append('none' if k == 0 else 'all' if k == min(width, keep.size - s) else 'mixed')
    return out


def filter_census(keep, sz):
    """tiles of the count / write kernels (one even for n = 0), kept entries per tile, and all / none / mixed per
    slice and per wave (relative to the entries the slice or wave really has)"""
    keep = np.asarray(keep, bool)
    n = keep.size
    tiles = ceil_div(max(n, 1), sz.filter_tile)
    return dict(tiles=tiles, tile_counts=[int(keep[t * sz.filter_tile:(t + 1) * sz.filter_tile].sum()) for t in range(tiles)],
                slices=_classes(keep, sz.filter_slice), waves=_classes(keep, WAVE), kept=int(keep.sum()),
                flag_blocks=ceil_div(n, 256))


FILTER_PATTERNS = ('none', 'all', 'first', 'last', 'alternating', 'lanes-0-63', 'wave-on-wave-off', 'slice-on-slice-off',
                   'random-1pct', 'random-50pct', 'random-99pct')


def filter_sizes(sz):
    T, s = sz.filter_tile, sz.filter_slice
    return (0, 1, WAVE - 1, WAVE, WAVE + 1, s - 1, s, s + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 300)


def keep_pattern(name, n, sz, seed=0):
    i = np.arange(n)
    if name == 'none':
        return np.zeros(n, bool)
    if name == 'all':
        return np.ones(n, bool)
    if name == 'first':
        return i == 0
    if name == 'last':
        return i == n - 1
    if name == 'alternating':
        return i % 2 == 0
    if name == 'lanes-0-63':
        return (i % WAVE == 0) | (i % WAVE == WAVE - 1)
    if name == 'wave-on-wave-off':
        return (i // WAVE) % 2 == 0
    if name == 'slice-on-slice-off':
        return (i // sz.filter_slice) % 2 == 0
    p = {'random-1pct': 0.01, 'random-50pct': 0.5, 'random-99pct': 0.99}[name]
    return np.random.default_rng(1000 + seed + n).random(n) < p


def filter_target_ok(name, n, census, sz):
    """the census a keep pattern is built for"""
    w, s = census['waves'], census['slices']
    if census['tiles'] != ceil_div(max(n, 1), sz.filter_tile) or sum(census['tile_counts']) != census['kept']:
        return False
    if name == 'none':
        return census['kept'] == 0 and all(x == 'none' for x in w)
    if name == 'all':
        return census['kept'] == n and all(x == 'all' for x in w)
    if name in ('first', 'last'):
        at = 0 if name == 'first' else len(w) - 1
        return census['kept'] == min(n, 1) and all((x != 'none') == (j == at) for j, x in enumerate(w))
    if name == 'alternating':
        return census['kept'] == (n + 1) // 2 and all(x == 'mixed' for x in w[:n // WAVE])
    if name == 'lanes-0-63':
        return census['kept'] == n // WAVE * 2 + (1 if n % WAVE else 0) and all(x == 'mixed' for x in w[:n // WAVE])
    if name == 'wave-on-wave-off':
        return all(x == ('all', 'none')[j % 2] for j, x in enumerate(w)) and all(x == 'mixed' for x in s[:n // sz.filter_slice])
    if name == 'slice-on-slice-off':
        return all(x == ('all', 'none')[j % 2] for j, x in enumerate(s))
    return census['kept'] == sum(census['tile_counts'])


def filter_inputs(pred, keep, variant, seed=0):
    """Inputs of predicate `pred` whose keep flags are exactly `keep`: dict(row, col, mask, map, a, b, M, N).  Rows are
    sorted; `variant` cycles through the parameters a predicate has (the range's position, the diagonal, the mask
    byte)."""
    keep = np.asarray(keep, bool)
    n = keep.size
    rng = np.random.default_rng(2000 + seed + 7 * n + variant)
    M, N = 60, 100
    row = np.sort(rng.integers(0, M, n)).astype(I64)
    col = rng.integers(0, N, n).astype(I64)
    mask = cmap = None
    a = b = 0
    byte = (1, 2, 255)[variant % 3]

    def choose(good):
        """col[i] from the columns with good[col] == keep[i]"""
        yes, no = np.flatnonzero(good), np.flatnonzero(~good)
        return np.where(keep, yes[rng.integers(0, yes.size, n)], no[rng.integers(0, no.size, n)]).astype(I64)

    if pred == 'col_range':
        if not keep.any() and variant % 2 == 0:
            a, b = (0, N // 2, N)[variant // 2 % 3], 0                 # b = 0 keeps nothing, wherever a is
        else:
            a, b = ((0, 40), (60, 40), (30, 40))[variant % 3]          # a at either end of the columns, and inside
            inside = (np.arange(N) >= a) & (np.arange(N) < a + b)
            col = choose(inside)
    elif pred == 'off_diag':
        a = (-3, 0, 5)[variant % 3]                                    # the diagonal k
        row = np.sort(rng.integers(max(0, -a), M, n)).astype(I64)
        other = rng.integers(1, N, n)
        col = np.where(keep, (row + a + other) % (N + M), row + a).astype(I64)
        col = np.where(keep & (col == row + a), col + 1, col)
    elif pred == 'mask':
        mask = np.where(keep, byte, 0).astype(np.uint8)
    elif pred == 'mask_row':
        # a new row wherever the flag changes (and at random), so that one byte per row gives exactly `keep`
        brk = np.concatenate(([0], (keep[1:] != keep[:-1]) | (rng.random(max(n - 1, 0)) < 0.3))) if n else np.zeros(0)
        row = np.cumsum(brk).astype(I64) + (variant % 3)
        M = int(row[-1]) + 2 if n else 2
        mask = np.zeros(M, np.uint8)
        mask[row[keep]] = byte
    elif pred == 'mask_col':
        good = rng.random(N) < 0.5
        good[:2] = (True, False)
        col = choose(good)
        mask = np.where(good, byte, 0).astype(np.uint8)
    elif pred == 'col_mapped':
        good = rng.random(N) < 0.5
        good[:2] = (True, False)
        cmap = np.full(N, -1, I64)
        ranks = np.arange(int(good.sum()), dtype=I64)
        ranks[-1] = (1 << 40) + 9                                      # -1, 0 and a large rank
        cmap[good] = ranks
        col = choose(good)
    else:
        raise ValueError(pred)
    got = keep_flags(pred, row, col, mask, cmap, a, b)
    assert np.array_equal(got, keep), (pred, n, variant)
    return dict(row=row, col=col, mask=mask, map=cmap, a=a, b=b, M=M, N=max(N, int(col.max()) + 1 if n else N))


def filter_cases(sz):
    """(id, n, pattern, variant) -- the same for every predicate"""
    out = []
    for j, n in enumerate(filter_sizes(sz)):
        for p, name in enumerate(FILTER_PATTERNS):
            out.append(('n%d-%s' % (n, name), n, name, j + p))
    return out


# ---------------------------------------------------------------------------------------------------------------
# scatter_rows (column-wise concatenation)
# ---------------------------------------------------------------------------------------------------------------
def cat_plan(rows, M):
    """rows: the sorted row ids of every operand -> (out_rowptr[M + 1], [delta[M] per operand])"""
    ptrs = [ind2ptr(r, M) for r in rows]
    counts = [np.diff(p) for p in ptrs]
    out_ptr = np.concatenate(([0], np.cumsum(sum(counts)))).astype(I64)
    deltas, before = [], np.zeros(M, I64)
    for p, c in zip(ptrs, counts):
        deltas.append((out_ptr[:-1] + before - p[:-1]).astype(I64))
        before = before + c
    return out_ptr, deltas


def cat_columns(ops, M):
    """ops: [(row, col, width)] sorted by (row, col) each -> (row, col, src) of [A | B | ...]: the concatenated
    entries with shifted columns, ordered by (row, col) with a stable sort; src counts through the operands."""
    row = np.concatenate([i64(r) for r, _, _ in ops])
    shift = np.cumsum([0] + [w for _, _, w in ops])
    col = np.concatenate([i64(c) + s for (_, c, _), s in zip(ops, shift)])
    order = np.lexsort((col, row))
    return row[order], col[order], order.astype(I64)


def scatter_cases(sz):
    """(id, M, [(row, col, width)])"""
    rng = np.random.default_rng(9)
    s = sz.filter_slice

    def pattern(M, N, n, rows=None):
        key = np.sort(rng.choice(M * N, n, replace=False))
        r, c = key // N, key % N
        if rows is not None:  # only these rows are non-empty
            r = np.sort(rows[rng.integers(0, rows.size, n)])
            c = np.concatenate([np.sort(rng.choice(N, int((r == x).sum()), replace=False)) for x in np.unique(r)]) if n else c
        return i64(r), i64(c), N

    M = 40
    even, odd = np.arange(0, M, 2), np.arange(1, M, 2)
    return [
        ('two-operands-n%d-n%d' % (s - 1, s + 1), M, [pattern(M, 30, s - 1), pattern(M, 50, s + 1)]),
        ('three-operands-n%d' % s, M, [pattern(M, 30, s), pattern(M, 7, 100), pattern(M, 50, 3 * s + 5)]),
        ('one-operand-empty', M, [pattern(M, 30, 200), pattern(M, 9, 0), pattern(M, 20, 300)]),
        ('rows-empty-in-one-operand', M, [pattern(M, 40, 300, rows=even), pattern(M, 40, 280, rows=odd),
                                          pattern(M, 40, 20, rows=np.array([0, M - 1]))]),
    ]


# ---------------------------------------------------------------------------------------------------------------
# diag
# ---------------------------------------------------------------------------------------------------------------
def num_diag(M, N, k):
    """entries (d, d + k) with 0 <= d < M and 0 <= d + k < N"""
    d = np.arange(M)
    return int(((d + k >= 0) & (d + k < N)).sum())


def diag_entries(M, N, k):
    d = np.arange(M, dtype=I64)
    d = d[(d + k >= 0) & (d + k < N)]
    return d, d + k


def _merge(row, col, src, E, M, N, k):
    """the entries given + the whole k-th diagonal (src = E + j), ordered by (row, col), stable: an entry given
    precedes the diagonal entry of the same place"""
    dr, dc = diag_entries(M, N, k)
    r, c = np.concatenate((i64(row), dr)), np.concatenate((i64(col), dc))
    s = np.concatenate((i64(src), E + np.arange(dr.size, dtype=I64)))
    order = np.lexsort((c, r))
    return r[order], c[order], s[order]


def non_diag_mask(row, col, M, N, k):
    """mask[E + num_diag]: 1 at the slot an off-diagonal entry takes once the whole diagonal is merged into the E
    entries; an entry ON the diagonal keeps its place in the count but gets no byte"""
    row, col = i64(row), i64(col)
    E = row.size
    _, _, s = _merge(row, col, np.arange(E), E, M, N, k)
    given = s < E
    on = np.zeros(s.size, bool)
    on[given] = col[s[given]] - row[s[given]] == k
    return (given & ~on).astype(np.uint8)


def insert_diag(row, col, M, N, k):
    """a pattern WITHOUT entries on the diagonal -> (row, col, src) of the merged pattern"""
    assert not (i64(col) - i64(row) == k).any()
    return _merge(row, col, np.arange(len(row)), len(row), M, N, k)


def set_diag(row, col, M, N, k):
    """plan + apply: -> (pos[E + 1], count, row, col, src): entries on the diagonal dropped, the whole diagonal in"""
    row, col = i64(row), i64(col)
    keep = keep_flags('off_diag', row, col, None, None, k, 0)
    pos, count = filter_positions(keep)
    src = np.flatnonzero(keep)
    r, c, s = _merge(row[src], col[src], src, row.size, M, N, k)  # diagonal entry j: E + j with E the INPUT size
    return pos, count, r, c, s


def diag_census(E, M, N, k):
    """blocks of the move kernel (one thread per entry) and of the fill kernel (one per diagonal entry)"""
    return dict(move=ceil_div(E, 256), fill=ceil_div(num_diag(M, N, k), 256))


def diag_pattern(M, N, k, kind, seed, density=0.4):
    """a sorted pattern that holds the 'whole' k-th diagonal, 'part' of it or 'none' of it"""
    rng = np.random.default_rng(seed)
    dense = rng.random((M, N)) < density
    dr, dc = diag_entries(M, N, k)
    if kind == 'whole':
        dense[dr, dc] = True
    elif kind == 'none':
        dense[dr, dc] = False
    else:
        assert kind == 'part'
        dense[dr, dc] = np.arange(dr.size) % 2 == 0
    r, c = np.nonzero(dense)
    return i64(r), i64(c)


def diag_small_cases():
    """(id, M, N, k, kind, row, col): every k from -(M + 1) to N + 1 on M < N, M = N, M > N, three kinds of pattern,
    E = 0, and one row with an entry immediately left and right of the diagonal place"""
    out = []
    for M, N in ((3, 6), (4, 4), (6, 2), (5, 5)):
        for k in range(-(M + 1), N + 2):
            for j, kind in enumerate(('whole', 'part', 'none')):
                r, c = diag_pattern(M, N, k, kind, 100 * M + 10 * N + k + j)
                out.append(('%dx%d-k%d-%s' % (M, N, k, kind), M, N, k, kind, r, c))
            z = np.zeros(0, I64)
            out.append(('%dx%d-k%d-E0' % (M, N, k), M, N, k, 'none', z, z))
    for k in (-1, 0, 1):
        d = 2
        out.append(('5x6-k%d-left-and-right-of-diagonal' % k, 5, 6, k, 'none', i64([0, d, d, 4]), i64([5, d + k - 1, d + k + 1, 0])))
        dr, dc = diag_entries(5, 6, k)
        key = np.sort(np.concatenate((dr * 6 + dc, [d * 6 + d + k - 1, d * 6 + d + k + 1])))
        out.append(('5x6-k%d-left-diagonal-right' % k, 5, 6, k, 'whole', i64(key // 6), i64(key % 6)))
    return out


DIAG_LARGE = (700, 900, (0, 1, -1, 200, -699, 899))


def diag_large_cases():
    """700 x 900 with a few thousand entries: more than one block in the move kernel, and in the fill kernel wherever
    the diagonal is longer than a block"""
    M, N, ks = DIAG_LARGE
    out = []
    for j, k in enumerate(ks):
        for kind in ('part', 'none'):
            r, c = diag_pattern(M, N, k, kind, 7000 + j, density=0.006)
            out.append(('%dx%d-k%d-%s' % (M, N, k, kind), M, N, k, kind, r, c))
    return out
