"""Reference of the SpSpMM value gradients (csrc/spspmm_bw.hip): an fp64 oracle written as plain loops over the
products, a tile-level restatement of what the balanced kernel does with an operand pair (the census), the operand
pairs at which it changes route, a piece-wise restatement of the kernel whose switches plant defects, and the one
comparator that the CPU and the GPU tests share.  numpy only.  Test infrastructure, not a conftest.

With C = A * B (structural pattern, rows sorted by column), gC the gradient of C's values, pos(i, j) the index of
(i, j) in C:

    gA[e] = sum_{p in row k of B}    vB[p] * gC[pos(i, colB[p])]      e = (i, k) of A
    gB[p] = sum_{e in column k of A} vA[e] * gC[pos(row(e), j)]       p = (k, j) of B

A missing value tensor counts as all ones.  Both sides are one computation (include/tsamd.h): a SEGMENT (entry of
A | entry of B) owns a LIST (row k of B | column k of A); ``generic`` puts a side into that form."""
import functools
import math
from collections import namedtuple

import numpy as np

from tests import spspmm_cases as sc

MAX_TILE = 4096  # the builders are sized for tiles up to this many products
NP_DT = {'f32': np.float32, 'f64': np.float64}
# the project's bounds of a floating sum (tests/util.py SUM_TOL / SUM_ATOL), repeated here so that this module needs
# no torch; test_spspmm_grad_reference.py asserts they are the same numbers
SUM_TOL = {'f32': 1e-5, 'f64': 1e-13}
SUM_ATOL = {'f32': 1e-37, 'f64': 1e-300}
DEFECTS = ('last_term_dropped', 'lookup_off_by_one', 'row_order_on_column_side', 'empty_unwritten',
           'missing_value_is_zero', 'carry_twice')


# ---- operand pairs -----------------------------------------------------------------------------------------------
def _csr(rows, ncols):
    """list of column-id lists -> (rowptr, col); every row sorted and unique."""
    rows = [np.unique(np.asarray(r, np.int64)) for r in rows]
    for r in rows:
        assert r.size == 0 or (r[0] >= 0 and r[-1] < ncols)
    rowptr = np.zeros(len(rows) + 1, np.int64)
    rowptr[1:] = np.cumsum([r.size for r in rows])
    col = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return rowptr, col.astype(np.int64)


def make_pair(name, a_rows, b_rows, N):
    K = len(b_rows)
    rowptrA, colA = _csr(a_rows, K)
    rowptrB, colB = _csr(b_rows, N)
    return finish_pair(dict(name=name, m=len(a_rows), k=K, N=N, rowptrA=rowptrA, colA=colA, rowptrB=rowptrB, colB=colB))


def finish_pair(case):
    """Adds the row ids, A's column view and the pattern of C to a dict with the CSR arrays of A and B."""
    m, k = case['m'], case['k']
    rpA, cA, rpB, cB = case['rowptrA'], case['colA'], case['rowptrB'], case['colB']
    case['rowA'] = np.repeat(np.arange(m, dtype=np.int64), np.diff(rpA))
    case['rowB'] = np.repeat(np.arange(k, dtype=np.int64), np.diff(rpB))
    perm = np.lexsort((case['rowA'], cA)).astype(np.int64)  # stable column-major order
    case['csr2cscA'] = perm
    colptr = np.zeros(k + 1, np.int64)
    np.add.at(colptr, cA + 1, 1)
    case['colptrA'] = np.cumsum(colptr)
    # products in expansion order (A entry order, then B entry order)
    cnt = rpB[cA + 1] - rpB[cA]
    ea = np.repeat(np.arange(cA.size, dtype=np.int64), cnt)
    off = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    pb = rpB[cA[ea]] + off
    case['prodA'], case['prodB'] = ea, pb
    prow, pcol = case['rowA'][ea], cB[pb]
    order = np.lexsort((pcol, prow))
    r, c = prow[order], pcol[order]
    keep = np.ones(r.size, bool)
    keep[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    rowC, colC = r[keep], c[keep]
    rowptrC = np.zeros(m + 1, np.int64)
    np.add.at(rowptrC, rowC + 1, 1)
    case['rowptrC'], case['colC'], case['rowC'] = np.cumsum(rowptrC), colC, rowC
    pos = np.empty(r.size, np.int64)
    pos[order] = np.cumsum(keep) - 1
    case['prodC'] = pos  # index in C of every product
    return case


def _tile(T):
    assert 64 <= T <= MAX_TILE and T % 64 == 0, 'the builders were sized for tiles of at most %d products' % MAX_TILE
    return int(T)


def long_row(T):
    """Row 3 of B has 3T + 5 entries; A (5 x 8) has entries in column 3 on rows 0, 2 and 4 and entries on short and
    empty B rows: the gA segments of column 3 span four tiles or more."""
    T = _tile(T)
    rng = np.random.default_rng(11)
    N = 4 * T + 64
    short = (2, 0, 5, None, 1, 0, 3, 4)  # entries of the rows of B; rows 1 and 5 are empty
    b_rows = [rng.choice(N, size=3 * T + 5, replace=False) if n is None else rng.choice(N, size=n, replace=False)
              for n in short]
    a_rows = [[0, 3, 5], [1, 2], [3], [], [1, 3, 4, 6, 7]]
    return make_pair('long_row', a_rows, b_rows, N)


def tall_col(T):
    """A has 3T + 5 rows, each with an entry in column 2 (a few with others too); row 2 of B has 3 entries: each of
    their gB segments has 3T + 5 terms."""
    T = _tile(T)
    rng = np.random.default_rng(12)
    m, K, N = 3 * T + 5, 6, 40
    a_rows = [[2] for _ in range(m)]
    for i in rng.choice(m, size=9, replace=False):
        a_rows[int(i)] = [2, int(rng.choice([0, 1, 3, 4, 5]))]
    b_rows = [[1, 7], [], [3, 20, 39], [0], [5, 6, 8, 30], [39]]
    return make_pair('tall_col', a_rows, b_rows, N)


def aligned(T):
    """Every row of B has exactly 64 entries and A has 3T/64 + 1 entries: every tile boundary of gA is a segment
    boundary."""
    T = _tile(T)
    rng = np.random.default_rng(13)
    K, N = 128, 4096
    b_rows = [rng.choice(N, size=64, replace=False) for _ in range(K)]
    n = 3 * T // 64 + 1
    per = -(-n // 4)
    assert per <= K
    a_rows, left = [], n
    for _ in range(4):
        take = min(per, left)
        a_rows.append(rng.choice(K, size=take, replace=False))
        left -= take
    return make_pair('aligned', a_rows, b_rows, N)


def _from_wide(name, N, lg_range, large):
    c = sc.make_case(N, lg_range, seed=0, large=large)
    case = dict(name=name, m=c['m'], k=c['k'], N=N, rowptrA=c['rowptrA'], colA=c['colA'], rowptrB=c['rowptrB'],
                colB=c['colB'], names=c['names'], wide_census=c['census'])
    return finish_pair(case)


def empties(T, lg_range):
    """tests/spspmm_cases.make_case without large rows: empty rows of A first, in the middle and last, a row over
    empty B rows only, rows of exactly 1 / 64 / 65 / 512 / 513 / 1024 products.  (On the column side almost every
    entry of B has an empty list: thousands of segments per tile.)"""
    _tile(T)
    return _from_wide('empties', 1 << 20, lg_range, 'none')


def wide(T, lg_range):
    """Column ids up to 2^32 - 3 = N - 1 (one hub row), as tests/test_spspmm_wide_gpu.py builds its widest operand."""
    _tile(T)
    return _from_wide('wide', 2 ** 32 - 2, lg_range, 'one')


def unstaged(T, limit):
    """The one further route of tsamd_spspmm_bw_route: a tile that intersects more than `limit` segments.  A has
    limit + 40 entries on EMPTY rows of B between entries on rows with products, on both sides of the run; B's
    productive rows are referenced from few rows of A, so that most entries of B have short lists and the entries of
    the unreferenced rows (more than `limit` of them in a run) have empty ones."""
    T = _tile(T)
    rng = np.random.default_rng(14)
    n_empty = limit + 40
    K, N = n_empty + 9, 3 * limit
    b_rows = [[] for _ in range(K)]
    for k in (0, 1, 2, 3):
        b_rows[k] = rng.choice(N, size=5 + k, replace=False)
    # rows K-5 .. K-2 of B: never referenced by A, limit + 40 entries together -> empty lists on the column side,
    # between the entries of rows 0 .. 3 and those of row K-1, which have products
    for j, k in enumerate(range(K - 5, K - 1)):
        b_rows[k] = rng.choice(N, size=n_empty // 4 + (j == 0) * (n_empty % 4), replace=False)
    b_rows[K - 1] = rng.choice(N, size=4, replace=False)
    empty_cols = np.arange(4, 4 + n_empty)  # empty rows of B
    half = n_empty // 2
    a_rows = [[0, 2], list(empty_cols[:half]) + [1], list(empty_cols[half:]) + [3], [0, 1, 2, 3, K - 1], []]
    return make_pair('unstaged', a_rows, b_rows, N)


@functools.lru_cache(maxsize=None)
def builders(T, limit, lg_range):
    """name -> case, every builder of the issue plus one per further route."""
    return {c['name']: c for c in (long_row(T), tall_col(T), aligned(T), empties(T, lg_range), wide(T, lg_range),
                                   unstaged(T, limit))}


# ---- values ------------------------------------------------------------------------------------------------------
def values(case, kind, seed=0):
    """(vA, vB, gC) as float64: spspmm_cases.values for the operands, the same two kinds for gC.  'dyadic':
    non-zero half-integers in [-2, 2], every sum exact in fp32; 'uniform': rounding-sensitive."""
    va, vb = sc.values(case, kind, seed)
    rng = np.random.default_rng([seed, 78, case['colC'].size])
    n = case['colC'].size
    if kind == 'dyadic':
        g = rng.integers(-4, 5, size=n) / 2.0
        # no zeros (as tests/test_spspmm_wide_gpu.py make_values): a term of -0.0 would make "bit-equal" a statement
        # about signed zeros -- a sum of non-zero terms that cancels is +0.0 in every order
        va[va == 0] = 0.5
        vb[vb == 0] = -1.5
        g[g == 0] = 1.0
    else:
        g = rng.random(n) - 0.5
        g[g == -0.5] = 0.25
    return va, vb, g


def stored(x, dtype):
    return None if x is None else np.asarray(x, np.float64).astype(NP_DT[dtype])


# ---- the generic form of a side ----------------------------------------------------------------------------------
Generic = namedtuple('Generic', 'segptr nrows segind listptr list_ind perm nseg')


def generic(case, side):
    """The operands of tsamd_spspmm_bw_plan / tsamd_spspmm_value_bw for a side; perm: list order -> entry of the
    operand that owns the list values (None: identity)."""
    if side == 0:
        return Generic(case['rowptrA'], case['m'], case['colA'], case['rowptrB'], case['colB'], None,
                       case['colA'].size)
    perm = case['csr2cscA']
    return Generic(case['rowptrB'], case['k'], case['colB'], case['colptrA'], case['rowA'][perm], perm,
                   case['colB'].size)


def list_lengths(case, side):
    g = generic(case, side)
    x = g.segind if side == 0 else (case['rowB'])
    return g.listptr[x + 1] - g.listptr[x]


# ---- oracle ------------------------------------------------------------------------------------------------------
def oracle(case, vA, vB, gC):
    """fp64 gradients by plain loops over the products: -> (gA, gB, l1A, l1B); l1 = sum |w * gC| per segment.  vA / vB
    None = all ones (the gradient of that side is then the gradient a tensor of ones would receive).  Every segment's
    terms are summed with math.fsum: the oracle carries no rounding of its own beyond the final one."""
    rpA, cA, rpB, cB, rpC, colC = (case[k] for k in ('rowptrA', 'colA', 'rowptrB', 'colB', 'rowptrC', 'colC'))
    gC = np.asarray(gC, np.float64)
    where = {}
    for i in range(case['m']):
        for z in range(int(rpC[i]), int(rpC[i + 1])):
            where[(i, int(colC[z]))] = z
    tA = [[] for _ in range(cA.size)]
    tB = [[] for _ in range(cB.size)]
    for i in range(case['m']):
        for e in range(int(rpA[i]), int(rpA[i + 1])):
            k = int(cA[e])
            a = 1.0 if vA is None else float(vA[e])
            for p in range(int(rpB[k]), int(rpB[k + 1])):
                b = 1.0 if vB is None else float(vB[p])
                g = float(gC[where[(i, int(cB[p]))]])
                tA[e].append(b * g)
                tB[p].append(a * g)
    fs = lambda lists: np.array([math.fsum(t) for t in lists], np.float64)  # noqa: E731
    ab = lambda lists: np.array([math.fsum(abs(x) for x in t) for t in lists], np.float64)  # noqa: E731
    return fs(tA), fs(tB), ab(tA), ab(tB)


# ---- census ------------------------------------------------------------------------------------------------------
Census = namedtuple('Census', 'P ntiles ptr tile_S tile_staged spans interior cut head tail runs ends_on_tile')


def _segment_of(ptr, nseg, e):
    """expand.h segment_of: the last i in [0, nseg) with ptr[i] <= e."""
    return np.searchsorted(ptr[:nseg], e, side='right') - 1


def census(case, side, T, limit):
    """What spspmm_bw_tile_kernel / spspmm_bw_fixup_kernel do with a side.  tile_S: segments a tile intersects
    (staged in LDS when <= limit).  spans: tiles a non-empty segment touches (0 for an empty one); interior: inside
    one tile; cut: crosses a tile boundary.  head / tail: the segment of a tile's head / tail record or -1.  runs:
    tail records the fix-up folds for a tile's head (0: no head).  ends_on_tile: a segment ends on a tile boundary."""
    lens = list_lengths(case, side)
    nseg = lens.size
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(ptr[-1])
    ntiles = -(-P // T)
    e0 = np.arange(ntiles, dtype=np.int64) * T
    e1 = np.minimum(e0 + T, P)
    fs, ls = _segment_of(ptr, nseg, e0), _segment_of(ptr, nseg, e1 - 1)
    S = ls - fs + 1
    first, last = ptr[:-1] // T, (ptr[1:] - 1) // T
    spans = np.where(lens > 0, last - first + 1, 0)
    head = np.where((ptr[fs] < e0) & (ptr[fs + 1] <= e1), fs, -1) if ntiles else np.zeros(0, np.int64)
    tail = np.where(ptr[ls + 1] > e1, ls, -1) if ntiles else np.zeros(0, np.int64)
    runs = np.zeros(ntiles, np.int64)
    for b in np.nonzero(head >= 0)[0]:
        i = b - 1
        while i >= 0 and tail[i] == head[b]:
            i -= 1
        runs[b] = b - 1 - i
    ends = ptr[1:][lens > 0]
    return Census(P, ntiles, ptr, S, S <= limit, spans, spans == 1, spans > 1, head, tail, runs,
                  bool((ends % T == 0).any()))


def assert_census(cases, T, limit):
    """Every builder reaches what it was built for: hard asserts, never skips."""
    assert T <= MAX_TILE
    c = {(n, s): census(cases[n], s, T, limit) for n in cases for s in (0, 1)}
    # long_row: the gA segments of column 3 of A span four tiles or more; short and empty lists beside them
    lr, cen = cases['long_row'], c[('long_row', 0)]
    hub = np.nonzero(lr['colA'] == 3)[0]
    assert hub.size == 3 and bool((np.diff(cen.ptr)[hub] == 3 * T + 5).all()) and bool((cen.spans[hub] >= 4).all())
    assert bool((cen.spans == 0).any()) and bool(cen.interior.any())
    assert bool((cen.runs >= 3).any()), 'no fix-up over three tail records'
    # tall_col: every gB segment of row 2 of B has 3T + 5 terms
    tc, cen = cases['tall_col'], c[('tall_col', 1)]
    hub = np.nonzero(tc['rowB'] == 2)[0]
    assert hub.size == 3 and bool((np.diff(cen.ptr)[hub] == 3 * T + 5).all()) and bool((cen.spans[hub] >= 4).all())
    assert bool((c[('tall_col', 0)].spans <= 2).all())
    # aligned: tile boundaries fall on segment boundaries, nothing is cut, no records
    cen = c[('aligned', 0)]
    assert cen.P == 3 * T + 64 and cen.ntiles == 4 and not cen.cut.any() and cen.ends_on_tile
    assert bool((cen.head == -1).all()) and bool((cen.tail == -1).all())
    assert bool((np.diff(cen.ptr) == 64).all())
    # empties: the named rows of the generator
    em, cen = cases['empties'], c[('empties', 0)]
    prod = em['wide_census']['products']
    names = em['names']
    for p in (1, 64, 65, 512, 513, 1024):
        assert prod[names.index('exact_%d' % p)] == p
    assert prod[0] == 0 and prod[-1] == 0 and prod[names.index('empty_middle')] == 0
    oe = names.index('only_empty_b')
    assert prod[oe] == 0 and em['rowptrA'][oe + 1] > em['rowptrA'][oe]
    assert bool((cen.spans == 0).any()) and cen.ntiles >= 2
    # wide: holds column N - 1 = 2^32 - 3, beyond signed 32-bit
    wd = cases['wide']
    assert wd['N'] == 2 ** 32 - 2 and int(wd['colC'].max()) == wd['N'] - 1 and int(wd['colB'].max()) == wd['N'] - 1
    assert bool((wd['colC'] >= 2 ** 31).any()) and wd['wide_census']['n_large'] == 1
    # the further route: tiles over more than `limit` segments, on either side, next to staged ones
    for side in (0, 1):
        cen = c[('unstaged', side)]
        assert bool((~cen.tile_staged).any()), 'side %d: no tile beyond %d segments' % (side, limit)
        assert cen.P > 0
    assert bool((~c[('empties', 1)].tile_staged).any()) and bool(c[('empties', 0)].tile_staged.all())
    for key in (('long_row', 0), ('long_row', 1), ('tall_col', 0), ('tall_col', 1), ('aligned', 0)):
        assert bool(c[key].tile_staged.all()), key
    return c


# ---- the kernel, piece by piece ----------------------------------------------------------------------------------
def emulate(case, side, w, gC, dtype, T, defect=None):
    """The balanced kernel restated: products in segment order, cut into tiles; every (segment, tile) piece is summed
    and rounded to `dtype` (tile kernel: written directly when the segment lies inside the tile, otherwise a carry
    record), the pieces of a cut segment fold in fp64 (fix-up).  w: the values of the list operand in ITS entry order
    (vB for side 0, vA for side 1) or None.  `defect` plants one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    g = generic(case, side)
    dt = NP_DT[dtype]
    lens = list_lengths(case, side)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    P = int(ptr[-1])
    out = np.zeros(g.nseg, dt)
    if defect == 'empty_unwritten':
        out[lens == 0] = np.nan  # whatever the buffer held
    if P == 0:
        return out
    seg = np.repeat(np.arange(g.nseg, dtype=np.int64), lens)
    t = np.arange(P, dtype=np.int64)
    fixed = (case['rowA'] if side == 0 else case['colB'])[seg]
    x0 = g.segind if side == 0 else case['rowB']
    q = g.listptr[x0][seg] + (t - ptr[seg])
    x = g.list_ind[q]
    row, col = (fixed, x) if side == 0 else (x, fixed)
    colC = case['colC']
    width = int(case['N']) + 1  # row * width + col < 2^63: rows < 2^31, columns < 2^32
    pos = np.searchsorted(case['rowC'] * width + colC, row * width + col)
    assert bool((colC[pos] == col).all())
    if defect == 'lookup_off_by_one':
        pos = np.minimum(pos + 1, colC.size - 1)
    if w is None:
        wt = np.zeros(P, dt) if defect == 'missing_value_is_zero' else np.ones(P, dt)
    else:
        w = np.asarray(w, dt)
        src = q if (g.perm is None or defect == 'row_order_on_column_side') else g.perm[q]
        wt = w[src]
    terms = (wt * np.asarray(gC, dt)[pos]).astype(np.float64)  # one rounding per product, as in the kernel
    if defect == 'last_term_dropped':
        terms[ptr[1:][lens > 0] - 1] = 0.0
    tile = t // T
    new = np.ones(P, bool)
    new[1:] = (seg[1:] != seg[:-1]) | (tile[1:] != tile[:-1])
    starts = np.nonzero(new)[0]
    piece = np.add.reduceat(terms, starts).astype(dt).astype(np.float64)
    pseg = seg[starts]
    first_piece = np.ones(starts.size, bool)
    first_piece[1:] = pseg[1:] != pseg[:-1]
    npieces = np.bincount(pseg, minlength=g.nseg)
    if defect == 'carry_twice':
        piece = np.where(first_piece & (npieces[pseg] > 1), 2.0 * piece, piece)
    tot = np.zeros(g.nseg, np.float64)
    np.add.at(tot, pseg, piece)
    out[lens > 0] = tot[lens > 0].astype(dt)
    return out


# ---- the comparator ----------------------------------------------------------------------------------------------
def check_grad(got, exact, l1, dtype, kind, tag=''):
    """`got`: a gradient in `dtype`.  'dyadic': the bits of the exact result (every sum is exact in the value type).
    'uniform': |got - exact| <= SUM_TOL * L1 + SUM_ATOL.  -> the largest err / bound."""
    got = np.asarray(got)
    assert got.dtype == NP_DT[dtype] and got.shape == exact.shape, '%s: %s %s, expected %s %s' % (
        tag, got.dtype, got.shape, NP_DT[dtype], exact.shape)
    assert not np.isnan(got).any(), '%s: NaN in the gradient' % tag
    if kind == 'dyadic':
        want = exact.astype(NP_DT[dtype])
        assert np.array_equal(want.astype(np.float64), exact), '%s: the reference is not exact in %s' % (tag, dtype)
        iv = np.int32 if dtype == 'f32' else np.int64
        bad = got.view(iv) != want.view(iv)
        assert not bad.any(), '%s: %d of %d gradients differ in bits, first at %d' % (
            tag, int(bad.sum()), bad.size, int(np.argmax(bad)))
        return 0.0
    assert kind == 'uniform'
    err = np.abs(got.astype(np.float64) - exact)
    bound = SUM_TOL[dtype] * l1 + SUM_ATOL[dtype]
    ratio = float((err / bound).max()) if err.size else 0.0
    assert ratio <= 1.0, '%s: max err / bound %.3g' % (tag, ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def expected(T, limit, lg_range, name, kind, dtype, mode):
    """Cached oracle of a builder on the values AS STORED in `dtype`: (vA, vB, gC, gA, gB, l1A, l1B).  mode: 'both' |
    'a_only' | 'b_only' (the other operand has no values)."""
    case = builders(T, limit, lg_range)[name]
    va, vb, g = values(case, kind)
    va = stored(va, dtype) if mode in ('both', 'a_only') else None
    vb = stored(vb, dtype) if mode in ('both', 'b_only') else None
    g = stored(g, dtype)
    f64 = lambda a: None if a is None else a.astype(np.float64)  # noqa: E731
    return (va, vb, g) + oracle(case, f64(va), f64(vb), f64(g))
