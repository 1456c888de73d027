"""Reference of the segmented softmax (csrc/softmax.hip): an fp64 oracle of the forward and the backward, the comparators
the GPU result has to pass, the layouts at which the kernels change route (sized from tsamd_segment_softmax_route) with
a host census of the route every segment takes, the value kinds, and a numpy softmax by pieces whose switches plant
defects.  numpy only (ctypes for the four route constants).

Element types are named 'f32' 'f64' 'f16' 'bf16'; a bf16 array is carried as its uint16 bits (tests/util.py)."""
import ctypes
import math
from collections import namedtuple

import numpy as np

from pytorch_sparse_amd import _native as nat
from tests.segreduce_reference import ACC, bits, from_acc, same_bits, store, to_acc  # noqa: F401

FLOATS = ('f32', 'f64', 'f16', 'bf16')
KINDS = ('normal', 'late_max', 'big', 'neg_inf_piece', 'all_neg_inf', 'nan_one_head', 'pos_inf')
MUTANTS = ('no_max', 'per_chunk', 'no_rescale', 'unguarded_identity', 'perm_read_only', 'shared_normaliser',
           'storage_sum', 'bw_no_dot')
U = {'f32': 2.0 ** -23, 'f16': 2.0 ** -23, 'bf16': 2.0 ** -23, 'f64': 2.0 ** -52}  # of the accumulator
TINY = {'f32': 2.0 ** -126, 'f16': 2.0 ** -126, 'bf16': 2.0 ** -126, 'f64': 2.0 ** -1022}  # its smallest normal

Case = namedtuple('Case', 'name ptr E nseg')


def route():
    """(CHUNK, TILE, STAGED, FOLD) as tsamd_segment_softmax_route reports them (host arithmetic only)."""
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_segment_softmax_route(out) == 0
    assert [int(x) for x in out[4:]] == [0, 0, 0, 0]
    return tuple(int(x) for x in out[:4])


CHUNK, TILE, STAGED, FOLD = route()


# ---- oracle ------------------------------------------------------------------------------------------------------
def _segments(ptr, nseg):
    ptr = np.asarray(ptr, np.int64)[:nseg + 1]
    assert nseg == 0 or (ptr[0] == 0 and bool((np.diff(ptr) >= 0).all()))
    lens = np.diff(ptr)
    ne = np.nonzero(lens > 0)[0]
    return ptr, ne, ptr[ne], lens[ne]


def _exact_sum(x, ptr, ne, starts, lens):
    """Per-segment sums of fp64 rows [E, D] -> [len(ne), D]; runs of more than 64 entries by math.fsum (a plain fp64
    loop over 70 000 entries carries more error than the fp64 kernel is allowed)."""
    out = np.add.reduceat(x, starts, axis=0) if ne.size else np.zeros((0, x.shape[1]))
    for k in np.nonzero(lens > 64)[0]:
        s, n = int(starts[k]), int(lens[k])
        for d in range(x.shape[1]):
            out[k, d] = math.fsum(x[s:s + n, d].tolist())
    return out


def _flat(a):
    return a.reshape(a.shape[0], int(np.prod(a.shape[1:], dtype=np.int64)))


def _order(perm, E):
    return np.arange(E, dtype=np.int64) if perm is None else np.asarray(perm, np.int64)


def forward_exact(value, perm, ptr, nseg):
    """value: numbers [E] or [E, *] in their own order.  -> (y64 in the same order and shape, |v - m| per entry, segment
    length per entry).  Per segment and head: m = max, y = exp(v - m) / fsum(exp(v - m)); numpy's own arithmetic gives
    the non-finite rules (-inf -> 0; only -inf, or a +inf, or a NaN -> all NaN)."""
    v = np.asarray(value, np.float64)
    shape = v.shape
    E = shape[0]
    v = _flat(v)
    p = _order(perm, E)
    ptr, ne, starts, lens = _segments(ptr, nseg)
    y = np.zeros_like(v)
    dist = np.zeros_like(v)
    n = np.ones(E, np.int64)
    if E:
        assert int(ptr[-1]) == E
        vs = v[p]
        with np.errstate(invalid='ignore', over='ignore'):
            m = np.repeat(np.maximum.reduceat(vs, starts, axis=0), lens, axis=0)
            ex = np.exp(vs - m)
            s = np.repeat(_exact_sum(ex, ptr, ne, starts, lens), lens, axis=0)
            y[p] = ex / s
            dist[p] = np.abs(vs - m)
        n[p] = np.repeat(lens, lens)
    return y.reshape(shape), dist.reshape(shape), n.reshape((E, ) + (1, ) * (len(shape) - 1))


def backward_exact(y, grad, perm, ptr, nseg):
    """From the STORED y and g (numbers, own order): -> (gv64, mass = y * (|g| + sum over the segment of y * |g|),
    segment length per entry)."""
    y, g = np.asarray(y, np.float64), np.asarray(grad, np.float64)
    shape = y.shape
    E = shape[0]
    y, g = _flat(y), _flat(g)
    p = _order(perm, E)
    ptr, ne, starts, lens = _segments(ptr, nseg)
    gv, mass = np.zeros_like(y), np.zeros_like(y)
    n = np.ones(E, np.int64)
    if E:
        ys, gs = y[p], g[p]
        with np.errstate(invalid='ignore', over='ignore'):
            dot = np.repeat(_exact_sum(gs * ys, ptr, ne, starts, lens), lens, axis=0)
            l1 = np.repeat(_exact_sum(np.abs(gs * ys), ptr, ne, starts, lens), lens, axis=0)
            gv[p] = ys * (gs - dot)
            mass[p] = np.abs(ys) * (np.abs(gs) + l1)
        n[p] = np.repeat(lens, lens)
    return gv.reshape(shape), mass.reshape(shape), n.reshape((E, ) + (1, ) * (len(shape) - 1))


# ---- comparators -------------------------------------------------------------------------------------------------
def _half_ulp(x, dtype):
    """Half an ulp of |x| rounded to a 16-bit storage type (0 for f32 / f64: the bound's u covers their store)."""
    if dtype == 'f16':
        with np.errstate(over='ignore', invalid='ignore'):
            return 0.5 * np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)
    if dtype == 'bf16':
        with np.errstate(divide='ignore'):
            e = np.floor(np.log2(np.abs(x)))
        return 0.5 * np.exp2(np.maximum(np.where(np.isfinite(e), e, -126.0), -126.0) - 7)
    return np.zeros_like(x)


def check_forward(got, value, perm, ptr, nseg, dtype, expect=None):
    """got / value: stored elements in their own order.  NaN exactly where the oracle has NaN, 0 wherever it has 0, and
    elsewhere |y - y64| <= (2 |v - m| + log2(max(n, 2)) + 8) u y64 + tiny (+ half an ulp of the stored result for the
    16-bit types).  -> the worst error / bound."""
    y64, dist, n = expect if expect is not None else forward_exact(to_acc(value, dtype), perm, ptr, nseg)
    g = to_acc(got, dtype).astype(np.float64)
    assert g.shape == y64.shape, 'shape %s, expected %s' % (g.shape, y64.shape)
    nan = np.isnan(y64)
    assert np.array_equal(np.isnan(g), nan), '%s: %d NaN positions differ' % (dtype, int((np.isnan(g) != nan).sum()))
    zero = y64 == 0
    assert bool((g[zero] == 0).all()), '%s: a zero of the oracle is not zero' % dtype
    ok = ~nan & ~zero
    with np.errstate(invalid='ignore'):
        bound = (2 * dist + np.log2(np.maximum(n, 2)) + 8) * U[dtype] * y64 + TINY[dtype] + _half_ulp(y64, dtype)
    ratio = float((np.abs(g - y64)[ok] / bound[ok]).max()) if ok.any() else 0.0
    assert ratio <= 1.0, '%s forward: max err / bound %.3g' % (dtype, ratio)
    return ratio


def check_backward(got, y, grad, perm, ptr, nseg, dtype, expect=None):
    """|gv - gv64| <= (log2(max(n, 2)) + 6) u y (|g| + sum_seg y |g|) + tiny (+ half an ulp for the 16-bit types); NaN
    exactly where the oracle has it."""
    gv64, mass, n = expect if expect is not None else backward_exact(to_acc(y, dtype), to_acc(grad, dtype), perm, ptr,
                                                                     nseg)
    g = to_acc(got, dtype).astype(np.float64)
    assert g.shape == gv64.shape
    nan = np.isnan(gv64)
    assert np.array_equal(np.isnan(g), nan), '%s: NaN positions of the gradient differ' % dtype
    ok = ~nan
    with np.errstate(invalid='ignore'):
        bound = (np.log2(np.maximum(n, 2)) + 6) * U[dtype] * mass + TINY[dtype] + _half_ulp(gv64, dtype)
    ratio = float((np.abs(g - gv64)[ok] / bound[ok]).max()) if ok.any() else 0.0
    assert ratio <= 1.0, '%s backward: max err / bound %.3g' % (dtype, ratio)
    return ratio


# ---- layouts -----------------------------------------------------------------------------------------------------
def _case(name, lens):
    lens = np.asarray(lens, np.int64)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Case(name, ptr, int(ptr[-1]), int(lens.size))


def _filler(rng, n):
    out = []
    while n > 0:
        k = min(int(rng.integers(1, 6)), n)
        out.append(k)
        n -= k
    return out


def _from_intervals(name, intervals, E, rng):
    lens, at = [], 0
    for s, e in sorted(intervals):
        assert s >= at and e > s
        lens += _filler(rng, s - at) + [e - s]
        at = e
    assert at <= E
    return _case(name, lens + _filler(rng, E - at))


LENGTHS = (1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1)
HUB = (FOLD + 2) * CHUNK + 1


def cases(seed=0):
    rng = np.random.default_rng(seed)
    out = [Case('no_segments', np.zeros(1, np.int64), 0, 0), _case('no_entries', [0] * 5), _case('single', [1])]
    lens = []
    for n in LENGTHS:
        lens += _filler(rng, 37) + [n]
    out.append(_case('lengths', lens + _filler(rng, 37)))
    out.append(_from_intervals('boundaries', [
        (2 * CHUNK + 100, 4 * CHUNK),  # cut, ends exactly on a chunk boundary
        (4 * CHUNK, 5 * CHUNK + 30),  # cut, starts exactly on one
        (6 * CHUNK - 10, 6 * CHUNK), (6 * CHUNK, 6 * CHUNK + 10),  # whole, on either side of one
        (TILE * 4 - 5, TILE * 4 + 5),  # cut by a tile boundary
    ], TILE * 4 + 300, rng))
    out.append(_case('hub', [3] * 50 + [HUB] + [3] * 50))
    lens = np.zeros(STAGED + 500, np.int64)
    lens[np.linspace(0, STAGED + 499, 10).astype(np.int64)] = 7
    out.append(_case('unstaged', lens.tolist() + _filler(rng, 3000)))
    out.append(_case('empties', [0] * 7 + _filler(rng, 700) + [0] * 9 + _filler(rng, 900) + [0] * 5))
    assert all(c.E < 100_000 for c in out)
    return out


# ---- census ------------------------------------------------------------------------------------------------------
Census = namedtuple('Census', 'seg_route seg_records tile_staged finish_chunks')


def census(case):
    """seg_route: 0 empty, 1 finished by the tile kernel (inside one chunk), 2 cut (fix-up + finish).  seg_records: tail
    records the fix-up folds for a cut segment.  tile_staged: does every tile's pointer slice fit LDS.  finish_chunks:
    chunks the finish kernel does not leave at once."""
    ptr, E, nseg = case.ptr, case.E, case.nseg
    lens = np.diff(ptr)
    first, last = ptr[:-1] // CHUNK, (ptr[1:] - 1) // CHUNK
    seg_route = np.where(lens == 0, 0, np.where(first == last, 1, 2))
    records = np.where(seg_route == 2, last - first, 0)
    e0 = np.arange(0, E, TILE, dtype=np.int64)
    e1 = np.minimum(e0 + TILE, E)
    seg_of = lambda e: np.searchsorted(ptr[:nseg], e, side='right') - 1  # noqa: E731
    staged = (seg_of(e1 - 1) - seg_of(e0) + 1) <= STAGED if E else np.zeros(0, bool)
    busy = np.zeros(-(-E // CHUNK), bool)
    for j in np.nonzero(seg_route == 2)[0]:
        busy[first[j]:last[j] + 1] = True
    return Census(seg_route, records, staged, busy)


def assert_reaches_every_route(case_list):
    cs = [census(c) for c in case_list]
    routes = np.concatenate([c.seg_route for c in cs])
    assert all(bool((routes == r).any()) for r in (0, 1, 2)), 'a segment route is not reached'
    rec = np.concatenate([c.seg_records for c in cs])
    assert bool((rec == 1).any()) and bool((rec > FOLD).any()), 'fix-up: one record, more than one round'
    assert any(bool((~c.tile_staged).any()) for c in cs) and any(bool(c.tile_staged.any()) for c in cs), 'staging'
    assert any(bool((~c.finish_chunks).any()) for c in cs) and any(bool(c.finish_chunks.any()) for c in cs)
    lens = np.concatenate([np.diff(c.ptr) for c in case_list])
    assert set(LENGTHS) <= set(lens.tolist()) and HUB in lens
    return cs


# ---- values ------------------------------------------------------------------------------------------------------
def values(case, kind, dtype, D=3, seed=0):
    """Stored elements [E, D] of `dtype`."""
    rng = np.random.default_rng([seed, KINDS.index(kind), case.E, case.nseg])
    E = case.E
    ptr, ne, starts, lens = _segments(case.ptr, case.nseg)
    x = rng.standard_normal((E, D)) * 8
    cut = (starts // CHUNK) != ((starts + lens - 1) // CHUNK)
    if kind == 'late_max':
        x[(starts + lens - 1)[lens > 1]] = 40.0
    elif kind == 'big':
        x = 95 + rng.standard_normal((E, D))
    elif kind == 'neg_inf_piece':
        x[rng.random((E, D)) < 0.1] = -np.inf
        for s, n in zip(starts[lens >= 3 * CHUNK], lens[lens >= 3 * CHUNK]):
            b = (s // CHUNK + 1) * CHUNK
            x[s:b] = -np.inf  # the first piece
            x[b + CHUNK:b + 2 * CHUNK] = -np.inf  # a whole chunk between finite ones
    elif kind == 'all_neg_inf':
        for k in np.nonzero(cut | (np.arange(ne.size) % 7 == 0))[0]:
            x[starts[k]:starts[k] + lens[k], k % D] = -np.inf
            if cut[k]:
                x[starts[k]:starts[k] + lens[k]] = -np.inf
    elif kind == 'nan_one_head' and E:
        k = int(np.argmax(lens))
        x[starts[k] + lens[k] // 2, 1 % D] = np.nan
    elif kind == 'pos_inf' and E:
        for k in set(range(0, ne.size, 5)) | {int(np.argmax(lens))}:
            x[starts[k] + int(rng.integers(0, lens[k])), k % D] = np.inf
    return store(x, dtype)


def grads(case, dtype, D=3, seed=1):
    rng = np.random.default_rng([seed, case.E, case.nseg])
    return store(rng.standard_normal((case.E, D)), dtype)


# ---- a numpy softmax by pieces, with planted defects ---------------------------------------------------------------
def emulate_forward(value, perm, ptr, nseg, dtype, mutant=None):
    """Stored elements in, stored elements out (own order).  Every segment is cut at the chunk boundaries, each piece
    reduced to (m, s) in the accumulator type, the pieces folded in entry order from the identity (-inf, 0) with the
    guarded online-softmax combine, every entry normalised by the result.  `mutant` plants one defect."""
    assert mutant is None or mutant in MUTANTS
    a = to_acc(value, dtype)
    A = a.dtype.type
    E = a.shape[0]
    a2 = _flat(a)
    p = _order(perm, E)
    ptr = np.asarray(ptr, np.int64)
    vs = a2[p] if E else a2
    ys = np.zeros_like(vs)
    ninf = A(-np.inf)

    def piece_sum(t):
        if mutant == 'storage_sum' and dtype in ('f16', 'bf16'):
            acc = np.zeros(t.shape[1], A)
            for row in t:  # rounded to the storage type after every addition
                acc = to_acc(from_acc(acc + row, dtype), dtype)
            return acc
        return t.sum(axis=0, dtype=A)

    def comb(m1, s1, m2, s2):
        m = np.where((m1 > m2) | np.isnan(m1), m1, m2)
        if mutant == 'no_rescale':
            return m, s1 + s2
        f1, f2 = np.exp(m1 - m), np.exp(m2 - m)
        if mutant != 'unguarded_identity':
            f1, f2 = np.where(m1 == ninf, A(0), f1), np.where(m2 == ninf, A(0), f2)
        return m, (s1 * f1 + s2 * f2).astype(A)

    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(nseg):
            s, e = int(ptr[j]), int(ptr[j + 1])
            if s == e:
                continue
            v = vs[s:e]
            if mutant == 'no_max':
                ex = np.exp(v)
                ys[s:e] = ex / ex.sum(axis=0, dtype=A)
                continue
            cuts = [s] + list(range((s // CHUNK + 1) * CHUNK, e, CHUNK)) + [e]
            m, tot = np.full(v.shape[1], ninf), np.zeros(v.shape[1], A)
            for b0, b1 in zip(cuts[:-1], cuts[1:]):
                t = vs[b0:b1]
                pm = t.max(axis=0)
                ex = np.exp(t - pm)
                if mutant != 'unguarded_identity':  # exp(-inf - -inf) counts as 0
                    ex = np.where(np.isneginf(t) & np.isneginf(pm), A(0), ex)
                ps = piece_sum(ex)
                if mutant == 'per_chunk':
                    ys[b0:b1] = ex / ps
                m, tot = comb(m, tot, pm, ps)
            if mutant == 'per_chunk':
                continue
            if mutant == 'shared_normaliser':
                m, tot = np.full_like(m, m[0]), np.full_like(tot, tot[0])
            ys[s:e] = np.exp(v - m) / tot
    y = np.zeros_like(ys)
    if E:
        if mutant == 'perm_read_only':
            y = ys
        else:
            y[p] = ys
    return from_acc(y.reshape(a.shape), dtype)


def emulate_backward(y, grad, perm, ptr, nseg, dtype, mutant=None):
    ya, ga = to_acc(y, dtype), to_acc(grad, dtype)
    A = ya.dtype.type
    E = ya.shape[0]
    y2, g2 = _flat(ya), _flat(ga)
    p = _order(perm, E)
    ptr, ne, starts, lens = _segments(ptr, nseg)
    out = np.zeros_like(y2)
    if E:
        ys, gs = y2[p], g2[p]
        with np.errstate(invalid='ignore', over='ignore'):
            dot = np.repeat(np.stack([(gs[s:s + n] * ys[s:s + n]).sum(axis=0, dtype=A) for s, n in zip(starts, lens)]),
                            lens, axis=0)
            out[p] = ys * gs if mutant == 'bw_no_dot' else ys * (gs - dot)
    return from_acc(out.reshape(ya.shape), dtype)
