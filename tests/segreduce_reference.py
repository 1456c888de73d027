"""Reference of the entry-balanced segmented reduction (csrc/segreduce.hip): an fp64 oracle, the sequential loop of
csrc/coalesce.hip restated in the accumulator type, the layouts at which the kernel changes route, a host census of
what its two kernels do with a layout, and a lane-level restatement of the kernel whose switches plant defects.
numpy only.

Element types are named 'f32' 'f64' 'f16' 'bf16' 'i32' 'i64'; a bf16 array is carried as its uint16 bits (the
convention of tests/util.py: tonp / fromnp)."""
import math
from collections import namedtuple

import numpy as np

WAVE, WINDOWS = 64, 8
CHUNK = WAVE * WINDOWS  # entries per wave
TILE = 2048  # entries per workgroup (kExpandTile); a tile stages at most TILE segments
FLOATS = ('f32', 'f64', 'f16', 'bf16')
INTS = ('i32', 'i64')
DTYPES = FLOATS + INTS
REDUCES = ('sum', 'mean', 'min', 'max')
ACC = {'f32': np.float32, 'f64': np.float64, 'f16': np.float32, 'bf16': np.float32, 'i32': np.int32, 'i64': np.int64}
KINDS = ('integers', 'uniform', 'signed_zero', 'nan')
MUTANTS = ('end_off_by_one', 'empty_at_init', 'mean_truncates', 'mean_by_chunk_count', 'carry_dropped',
           'fold_at_most_64', 'nan_tree_rule', 'ties_to_later')

Case = namedtuple('Case', 'name ptr E nseg')


# ---- element types ----------------------------------------------------------------------------------------------
def to_acc(a, dtype):
    """Stored elements -> Traits<T>::acc_t."""
    a = np.asarray(a)
    if dtype == 'bf16':
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(ACC[dtype])


def from_acc(a, dtype):
    """Traits<T>::from_acc: one rounding to the element type (bf16: nearest even, NaN -> 0x7FC0)."""
    a = np.asarray(a, ACC[dtype])
    if dtype == 'f16':
        with np.errstate(over='ignore'):
            return a.astype(np.float16)
    if dtype == 'bf16':
        u = np.ascontiguousarray(a).view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        r[np.isnan(a)] = 0x7FC0
        return r
    return a


def store(x, dtype):
    """fp64 / int64 numbers -> stored elements of `dtype` (rounded once)."""
    with np.errstate(over='ignore'):
        return from_acc(np.asarray(x).astype(ACC[dtype]), dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


# ---- oracle ------------------------------------------------------------------------------------------------------
def _segmented(value, perm, ptr, nseg):
    """-> (entries in segmented order as [E, D], ptr[:nseg + 1], trailing shape).  ptr[0] must be 0."""
    ptr = np.asarray(ptr, np.int64)[:nseg + 1]
    assert ptr[0] == 0 and bool((np.diff(ptr) >= 0).all())
    v = np.asarray(value)
    tail = v.shape[1:]
    if perm is not None:
        v = v[np.asarray(perm, np.int64)]
    v = v.reshape(v.shape[0], -1)[:int(ptr[-1])]
    return v, ptr, tail


def _nonempty(ptr):
    lens = np.diff(ptr)
    ne = np.nonzero(lens > 0)[0]
    return ne, ptr[ne], lens[ne]


def _exact_sum(v, ptr):
    """Per-segment sums of fp64 / int64 rows.  Runs of more than 64 floats are summed with math.fsum: a plain fp64
    loop over 66 000 entries would carry more error than the fp64 kernel is allowed."""
    ne, starts, lens = _nonempty(ptr)
    out = np.zeros((len(ptr) - 1, v.shape[1]), v.dtype)
    if ne.size:
        out[ne] = np.add.reduceat(v, starts, axis=0)
    if v.dtype.kind == 'f':
        for j in ne[lens > 64]:
            for d in range(v.shape[1]):
                out[j, d] = math.fsum(v[ptr[j]:ptr[j + 1], d].tolist())
    return out


def reduce_exact(value, perm, ptr, nseg, reduce):
    """value: numbers (already in a numpy numeric type).  Floats -> (fp64 result, L1 mass of sum / mean = sum |v| over
    the segment, divided by the count for mean; None for min / max); integers -> (int64 result, None), mean by floor
    division.  Empty segments: 0."""
    v, ptr, tail = _segmented(value, perm, ptr, nseg)
    floating = v.dtype.kind == 'f'
    v = v.astype(np.float64 if floating else np.int64)
    ne, starts, lens = _nonempty(ptr)
    cnt = np.maximum(np.diff(ptr), 1)[:, None]
    if reduce in ('sum', 'mean'):
        out = _exact_sum(v, ptr)
        l1 = _exact_sum(np.abs(v), ptr) if floating else None
        if reduce == 'mean':
            out = out / cnt if floating else np.floor_divide(out, cnt)
            l1 = l1 / cnt if floating else None
    else:
        out = np.zeros((nseg, v.shape[1]), v.dtype)
        if ne.size:
            out[ne] = (np.minimum if reduce == 'min' else np.maximum).reduceat(v, starts, axis=0)
        l1 = None
    shape = (nseg, ) + tail
    return out.reshape(shape), (None if l1 is None else l1.reshape(shape))


def _winner_loop(column, ptr, reduce):
    """The loop of segment_reduce_kernel, literally, on one column: -> winning entry of every non-empty segment.
    acc starts at the first value; `v < acc ? v : acc` -- a later NaN never wins, a NaN first stays, ties keep the
    earlier entry."""
    x = column.tolist()
    win = []
    for j in range(len(ptr) - 1):
        s, e = int(ptr[j]), int(ptr[j + 1])
        if s >= e:
            continue
        w, acc = s, x[s]
        if reduce == 'min':
            for i in range(s + 1, e):
                if x[i] < acc:
                    w, acc = i, x[i]
        else:
            for i in range(s + 1, e):
                if x[i] > acc:
                    w, acc = i, x[i]
        win.append(w)
    return np.asarray(win, np.int64)


def _winner(a, ptr, reduce):
    """The same winners for every column at once: the first entry when it is NaN, otherwise the leftmost entry that
    equals the extremum of the segment's non-NaN entries (test_segreduce_reference.py holds this to _winner_loop)."""
    ne, starts, lens = _nonempty(ptr)
    E = a.shape[0]
    pos = np.arange(E, dtype=np.int64)
    seg = np.repeat(np.arange(ne.size), lens)
    first = np.zeros(E, bool)
    first[starts] = True
    w = a
    if a.dtype.kind == 'f':
        w = np.where(np.isnan(a) & ~first[:, None], np.inf if reduce == 'min' else -np.inf, a)
    m = (np.minimum if reduce == 'min' else np.maximum).reduceat(w, starts, axis=0)
    hit = w == m[seg]
    if a.dtype.kind == 'f':
        hit |= first[:, None] & np.isnan(a)
    return np.minimum.reduceat(np.where(hit, pos[:, None], E), starts, axis=0)


def _sum_loop(a, ptr):
    """acc = first; acc += v, entry by entry, in a's own type."""
    ne, starts, lens = _nonempty(ptr)
    acc = a[starts].copy()
    for k in range(1, int(min(lens.max(), 64)) if ne.size else 0):
        act = lens > k
        acc[act] = acc[act] + a[starts[act] + k]
    for i in np.nonzero(lens > 64)[0]:
        rest = a[starts[i] + 64:starts[i] + lens[i]]
        acc[i] = np.add.accumulate(np.concatenate([acc[i:i + 1], rest]), axis=0)[-1]
    return acc


def _finish_mean(acc, cnt, truncate=False):
    if acc.dtype.kind == 'f':
        return acc / cnt.astype(acc.dtype)
    c = cnt.astype(acc.dtype)
    if truncate:
        return (np.sign(acc) * (np.abs(acc) // c)).astype(acc.dtype)
    return np.floor_divide(acc, c)


def reduce_sequential(value, perm, ptr, nseg, reduce, dtype):
    """segment_reduce_kernel of csrc/coalesce.hip restated: stored elements in, stored elements out; the accumulator
    is Traits<T>::acc_t and the result is rounded once on write."""
    v, ptr, tail = _segmented(value, perm, ptr, nseg)
    a = to_acc(v, dtype)
    ne, starts, lens = _nonempty(ptr)
    out = np.zeros((nseg, a.shape[1]), a.dtype)
    if ne.size:
        if reduce in ('min', 'max'):
            out[ne] = np.take_along_axis(a, _winner(a, ptr, reduce), axis=0)
        else:
            with np.errstate(over='ignore', invalid='ignore'):
                acc = _sum_loop(a, ptr)
                out[ne] = _finish_mean(acc, lens[:, None]) if reduce == 'mean' else acc
    return from_acc(out, dtype).reshape((nseg, ) + tail)


# ---- layouts -----------------------------------------------------------------------------------------------------
def _case(name, lens):
    lens = np.asarray(lens, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Case(name, ptr, int(ptr[-1]), int(lens.size))


def _filler(rng, n):
    """Segment lengths 1..5 that add up to n."""
    out = []
    while n > 0:
        k = min(int(rng.integers(1, 6)), n)
        out.append(k)
        n -= k
    return out


def _from_intervals(name, intervals, E, rng):
    """The given [start, end) segments, everything between them filled with short segments."""
    lens, at = [], 0
    for s, e in sorted(intervals):
        assert s >= at and e > s
        lens += _filler(rng, s - at) + [e - s]
        at = e
    assert at <= E
    return _case(name, lens + _filler(rng, E - at))


RULER_OFFSETS = (63, 64, 65, 511, 512, 513, 2047, 2048, 2049)


def _ruler(rng):
    """A segment END at each offset from a tile start; its START in the same window, then in the window, the chunk
    and the tile before the one that holds its last entry."""
    iv, t = [], 1
    for off in RULER_OFFSETS:
        for unit in (0, WAVE, CHUNK, TILE):
            end = t * TILE + off
            last = end - 1
            start = end - 3 if unit == 0 else last // unit * unit - 7
            iv.append((start, end))
            t += 3 if off > 2040 else 2
    return _from_intervals('ruler', iv, t * TILE + 77, rng)


def _long(name, rng, mid):
    """Segments the fix-up finishes after exactly 1, 63, 64, 65 and 129 chunks, starting on a chunk boundary
    (mid = 0: the first one at entry 0) or `mid` entries into a chunk; the last one ends on the last entry."""
    iv, c = [], 0
    for run in (1, 63, 64, 65, 129):
        iv.append((c * CHUNK + mid, (c + run) * CHUNK + 100))
        c += run + 1
    return _from_intervals(name, iv, iv[-1][1], rng)


TAIL_SIZES = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)


def gate_case(E, seed=5):
    """One segment of E - 1000 entries among short ones: the layout of the tests on either side of the operator's
    E >= 32768 gate."""
    return _from_intervals('gate%d' % E, [(300, E - 700)], E, np.random.default_rng(seed))


def cases(seed=0):
    rng = np.random.default_rng(seed)
    out = [_ruler(rng)]
    n = 3 * TILE + 100
    out.append(_case('ones', np.ones(n, np.int64)))
    lens = np.ones(n + 1, np.int64)
    lens[TILE + 1000] = 0  # 2049 segments meet the second tile
    out.append(_case('ones_plus_empty', lens))
    out.append(_case('empties_leading', [0] * 5000 + _filler(rng, 5000)))
    out.append(_case('empties_trailing', _filler(rng, 5000) + [0] * 5000))
    out.append(_case('empties_inside', _filler(rng, TILE + 700) + [0] * 3000 + _filler(rng, 2 * TILE - 700 + 33)))
    out.append(_case('one_segment', [5000]))
    out.append(_long('long_aligned', rng, 0))
    out.append(_long('long_mid', rng, 200))
    for E in TAIL_SIZES:
        out.append(_case('tail%d' % E, _filler(rng, E)))
    assert all(c.E <= 200_000 for c in out)
    return out


# ---- values ------------------------------------------------------------------------------------------------------
def values(case, kind, dtype, reduce='min', D=3, seed=0):
    """Stored elements [E, D] of `dtype` for a case.  `reduce` matters to 'signed_zero' alone (the tie has to be the
    extremum: the other entries are positive for min, negative for max)."""
    rng = np.random.default_rng([seed, KINDS.index(kind), case.E, case.nseg])
    E = case.E
    ne, starts, lens = _nonempty(case.ptr)
    if kind == 'integers':
        return store(rng.integers(-8, 9, (E, D)), dtype)
    assert dtype in FLOATS
    if kind == 'uniform':
        return store(rng.uniform(-1.0, 1.0, (E, D)), dtype)
    if kind == 'signed_zero':
        x = rng.integers(1, 9, (E, D)).astype(np.float64)
        third = np.maximum(lens // 3, 1)[:, None]
        p1 = starts[:, None] + (rng.random((ne.size, D)) * third).astype(np.int64)
        p2 = (starts + lens - 1)[:, None] - (rng.random((ne.size, D)) * third).astype(np.int64)
        sign = np.where(rng.random((ne.size, D)) < 0.5, -1.0, 1.0)
        cols = np.broadcast_to(np.arange(D), p1.shape)
        x[p2, cols] = -0.0 * sign
        x[p1, cols] = 0.0 * sign  # the earlier one, written last so that it survives a collision
        return store(-x if reduce == 'max' else x, dtype)
    assert kind == 'nan'
    x = rng.integers(-250, 251, (E, D)).astype(np.float64)  # exact in bf16, rarely equal
    for d in range(D):
        pat = (np.arange(ne.size) + d) % 6
        x[starts[(pat == 0) | (pat == 5)], d] = np.nan  # first
        mid = (pat == 1) | (pat == 5)
        x[starts[mid] + lens[mid] // 2, d] = np.nan  # middle
        x[starts[pat == 2] + lens[pat == 2] - 1, d] = np.nan  # last
        for s, n in zip(starts[pat == 3], lens[pat == 3]):  # all
            x[s:s + n, d] = np.nan
        for j in np.nonzero(lens >= 3 * WAVE)[0]:
            s, n = int(starts[j]), int(lens[j])
            w = (s // WAVE + 1 + (j + d) % 2) * WAVE  # a whole window of NaN between finite ones
            if w + 2 * WAVE <= s + n:
                x[w:w + WAVE, d] = np.nan
            for c in range((s // CHUNK + 1) * CHUNK, s + n, CHUNK)[(j + d) % 3::3]:  # first entry of a later chunk
                x[c, d] = np.nan
    return store(x, dtype)


# ---- census ------------------------------------------------------------------------------------------------------
Census = namedtuple('Census', 'tile_S tile_staged chunk_head chunk_tail chunk_run seg_writer idle_waves end_kinds')


def _segment_of(ptr, nseg, e):
    """expand.h segment_of: the last i in [0, nseg) with ptr[i] <= e."""
    return np.searchsorted(ptr[:nseg], e, side='right') - 1


def census(case):
    """What segreduce_tile_kernel and segreduce_fixup_kernel do with a layout.
    tile_S / tile_staged: pointer slice of every tile and whether it fits LDS.  chunk_head / chunk_tail: the segment
    of the chunk's head / tail record or -1.  chunk_run: tail records the fix-up folds for the chunk's head (0: no
    head).  seg_writer: 0 empty, 1 tile kernel, 2 fix-up.  idle_waves: waves with c0 >= e1.  end_kinds: segment ends
    on a (window, chunk, tile) boundary."""
    ptr, E, nseg = case.ptr, case.E, case.nseg
    e0 = np.arange(0, E, TILE, dtype=np.int64)
    e1 = np.minimum(e0 + TILE, E)
    S = _segment_of(ptr, nseg, e1 - 1) - _segment_of(ptr, nseg, e0) + 1
    c0 = np.arange(0, E, CHUNK, dtype=np.int64)
    c1 = np.minimum(c0 + CHUNK, E)
    fs, ls = _segment_of(ptr, nseg, c0), _segment_of(ptr, nseg, c1 - 1)
    head = np.where((ptr[fs] < c0) & (ptr[fs + 1] <= c1), fs, -1)
    tail = np.where(ptr[ls + 1] > c1, ls, -1)
    run = np.zeros(c0.size, np.int64)
    for b in np.nonzero(head >= 0)[0]:
        i = b - 1
        while i >= 0 and tail[i] == head[b]:
            i -= 1
        run[b] = b - 1 - i
    lens = np.diff(ptr)
    one_chunk = ptr[:-1] // CHUNK == (ptr[1:] - 1) // CHUNK
    writer = np.where(lens == 0, 0, np.where(one_chunk, 1, 2))
    waves = -(-(E - int(e0[-1])) // CHUNK) if E else 0
    ends = ptr[1:][lens > 0]
    kinds = tuple(bool((ends % u == 0).any()) for u in (WAVE, CHUNK, TILE))
    return Census(S, S <= TILE, head, tail, run, writer, TILE // CHUNK - waves if E else 0, kinds)


def assert_reaches_every_route(case_list):
    cs = [census(c) for c in case_list]
    assert any(bool(((c.tile_S == TILE) & c.tile_staged).any()) for c in cs), 'no staged tile with S == 2048'
    assert any(bool((~c.tile_staged).any()) for c in cs), 'no unstaged tile'
    assert any(bool(((c.chunk_head >= 0) & (c.chunk_tail >= 0)).any()) for c in cs), 'no chunk with head and tail'
    runs = np.concatenate([c.chunk_run for c in cs])
    for r in (0, 1, 63, 64, 65):
        assert bool((runs == r).any()), 'no fix-up run of exactly %d chunks' % r
    assert bool((runs >= 129).any()), 'no fix-up run of 129 chunks or more'
    for k, name in enumerate(('window', 'chunk', 'tile')):
        assert any(c.end_kinds[k] for c in cs), 'no segment end on a %s boundary' % name
    assert any(c.idle_waves > 0 for c in cs), 'no idle wave'
    return cs


# ---- the kernel, lane by lane ------------------------------------------------------------------------------------
def emulate_balanced(value, perm, ptr, nseg, reduce, dtype, mutant=None):
    """segreduce_tile_kernel + segreduce_fixup_kernel restated: the 6-step segmented scan of every window, the carry
    between the windows of a chunk, head / tail records, the fold of the tail records.  Min / max of floats follow the
    rule of the sequential loop: a NaN that is not its segment's first entry is neutralised on load, every combine is
    (earlier, later) and keeps the earlier piece on a tie.  `mutant` plants one defect (MUTANTS)."""
    assert mutant is None or mutant in MUTANTS
    v, ptr, tail_shape = _segmented(value, perm, ptr, nseg)
    true_ptr = ptr
    E, D = v.shape
    a = to_acc(v, dtype).copy()
    A = a.dtype
    red = 'sum' if reduce == 'mean' else reduce
    floating = A.kind == 'f'
    if mutant == 'end_off_by_one':
        ptr = ptr.copy()
        ptr[1:-1] = np.minimum(ptr[1:-1] + 1, E)
    lens = np.diff(ptr)
    init = 0
    if mutant == 'empty_at_init' and red != 'sum':
        lim = np.finfo(A) if floating else np.iinfo(A)
        init = lim.max if red == 'min' else lim.min
    out = np.full((nseg, D), init, A)
    if E == 0:
        return from_acc(out, dtype).reshape((nseg, ) + tail_shape)

    def comb(x, y):  # x: the earlier piece
        if red == 'sum':
            return x + y
        if mutant == 'ties_to_later':
            return np.where(y <= x if red == 'min' else y >= x, y, x)
        return np.where(y < x if red == 'min' else y > x, y, x)

    def finish(acc, segs, cnt=None):
        if reduce != 'mean':
            return acc
        cnt = lens[segs] if cnt is None else cnt
        return _finish_mean(acc, np.reshape(cnt, (-1, 1)), truncate=mutant == 'mean_truncates')

    seg = np.repeat(np.arange(nseg, dtype=np.int64), lens)
    if floating and red != 'sum' and mutant != 'nan_tree_rule':
        later = np.arange(E) != ptr[seg]
        a[np.isnan(a) & later[:, None]] = np.inf if red == 'min' else -np.inf
    nch = -(-E // CHUNK)
    pad = nch * CHUNK - E
    lane = np.arange(WAVE)
    sg = np.concatenate([seg, np.full(pad, -1, np.int64)]).reshape(nch, WINDOWS, WAVE)
    valid = sg >= 0
    sg = np.where(valid, sg, -2 - lane)  # invalid lanes never match a neighbour
    val = np.concatenate([a, np.zeros((pad, D), A)]).reshape(nch, WINDOWS, WAVE, D)
    pos = np.arange(nch * CHUNK, dtype=np.int64).reshape(nch, WINDOWS, WAVE)
    send = np.where(valid, ptr[np.maximum(sg, 0) + 1], 0)
    sstart = np.where(valid, ptr[np.maximum(sg, 0)], 0)
    c0 = np.arange(nch, dtype=np.int64) * CHUNK
    c1 = np.minimum(c0 + CHUNK, E)
    with np.errstate(over='ignore', invalid='ignore'):
        for off in (1, 2, 4, 8, 16, 32):
            ov = np.roll(val, off, axis=2)
            same = (np.roll(sg, off, axis=2) == sg) & (lane >= off)
            val = np.where(same[..., None], comb(ov, val), val)
        cseg = np.full(nch, -1, np.int64)
        cval = np.zeros((nch, D), A)
        hseg = np.full(nch, -1, np.int64)
        hval = np.zeros((nch, D), A)
        for w in range(WINDOWS):
            vw, sw, ok = val[:, w], sg[:, w], valid[:, w]
            if mutant != 'carry_dropped':
                carry = ok & (sw == cseg[:, None])
                vw = np.where(carry[..., None], comb(cval[:, None, :], vw), vw)
            is_end = ok & (pos[:, w] + 1 == send[:, w])
            mine = is_end & (sstart[:, w] >= c0[:, None])
            out[sw[mine]] = finish(vw[mine], sw[mine])
            heads = is_end & ~mine
            ch = np.nonzero(heads.any(axis=1))[0]
            hl = heads[ch].argmax(axis=1)
            hseg[ch], hval[ch] = sw[ch, hl], vw[ch, hl]
            act = np.nonzero(c0 + w * WAVE < c1)[0]
            last = np.minimum(c1[act] - (c0[act] + w * WAVE), WAVE) - 1
            cseg[act] = np.where(is_end[act, last], -1, sw[act, last])
            cval[act] = vw[act, last]
        for b in np.nonzero(hseg >= 0)[0]:
            s, run = hseg[b], 0
            while b - 1 - run >= 0 and cseg[b - 1 - run] == s:
                run += 1
            if mutant == 'fold_at_most_64':
                run = min(run, 64)
            tails = cval[b - run:b]
            if red == 'sum':  # fp32 partial sums fold in fp64
                tot = (tails.astype(np.float64 if A == np.float32 else A).sum(axis=0) + hval[b]).astype(A)
            else:
                tot = hval[b]
                if run:
                    acc = tails[0]
                    for t in tails[1:]:
                        acc = comb(acc, t)
                    tot = comb(acc, hval[b])
            cnt = ptr[s + 1] - c0[b] if mutant == 'mean_by_chunk_count' else None
            out[s] = finish(tot[None], np.asarray([s]), cnt)[0]
    if mutant == 'end_off_by_one':
        assert not np.array_equal(ptr, true_ptr)
    return from_acc(out, dtype).reshape((nseg, ) + tail_shape)


# ---- the comparator ----------------------------------------------------------------------------------------------
def check_result(got, value, perm, ptr, nseg, reduce, dtype, kind, sum_tol=None, sum_atol=None, expect=None):
    """`got`: stored elements.  'integers': the bits of the exact result rounded once.  min / max of any kind: the bits
    of the sequential loop.  'uniform' sum / mean: |got - exact| <= sum_tol * L1 + sum_atol.  `expect` caches
    reference(...) between calls."""
    ref = expect if expect is not None else reference(value, perm, ptr, nseg, reduce, dtype, kind)
    got = np.asarray(got)
    assert got.shape == ref[0].shape, 'shape %s, expected %s' % (got.shape, ref[0].shape)
    if kind == 'integers' or reduce in ('min', 'max'):
        bad = bits(got) != bits(ref[0])
        assert not bad.any(), '%s %s %s: %d outputs differ in bits, first at %s' % (
            dtype, reduce, kind, int(bad.sum()), np.argwhere(bad)[0])
        return 0.0
    assert kind == 'uniform', 'sum / mean of %s values has no expectation' % kind
    exact, l1 = ref
    err = np.abs(to_acc(got, dtype).astype(np.float64) - exact)
    bound = sum_tol * l1 + sum_atol
    assert not np.isnan(err).any(), '%s %s: NaN in the result' % (dtype, reduce)
    ratio = float((err / bound).max()) if err.size else 0.0
    assert ratio <= 1.0, '%s %s: max err / bound %.3g' % (dtype, reduce, ratio)
    return ratio


def reference(value, perm, ptr, nseg, reduce, dtype, kind):
    """What check_result compares with: (stored bits, ) or (fp64 exact, L1)."""
    if reduce in ('min', 'max'):
        return (reduce_sequential(value, perm, ptr, nseg, reduce, dtype), )
    if kind == 'integers':
        exact, _ = reduce_exact(to_acc(value, dtype), perm, ptr, nseg, reduce)
        return (store(exact, dtype), )
    return reduce_exact(to_acc(value, dtype), perm, ptr, nseg, reduce)
