"""Reference of sparse attention (csrc/sddmm.hip, csrc/spmm_heads.hip): fp64 oracles of the multi-head SDDMM, the
multi-head SpMM and their four gradients written as loops over the entries, the comparators the GPU results have to
pass, layouts sized from the two route queries with a host census of what every row meets, and a numpy restatement by
pieces of the lane / chunk / record / fix-up scheme whose switches plant defects.  numpy only (ctypes for the routes).

Element types are named 'f32' 'f64' 'f16' 'bf16'; a bf16 array is carried as its uint16 bits (tests/util.py).

Comparators (derived, not tuned).  Every output is a sum of n products t_j.  An accumulator of unit roundoff u that adds
them in ANY order, each product rounded once at most, is off by at most (n - 1 + 1) u sum|t_j| to first order; the scale
of the SDDMM / the fp64 -> fp32 step of the SpMM fix-up and the conversion of `scale` to the accumulator type are two
more roundings: |got - exact| <= (n + 2) u sum|t_j|.  n = D for a score; for the SpMM n = 2 * (segment length): the
product's own rounding is counted as a term of its own, as is the ceiling for any summation order.  Gradual underflow
of a product loses at most one subnormal step each (n * tiny).  The 16-bit types round that accumulator once more:
half an ulp of the stored type at |exact| + bound.  u = 2^-24 (fp32 accumulator), 2^-53 (fp64)."""
import ctypes
from collections import namedtuple

import numpy as np

from pytorch_sparse_amd import _native as nat
from tests.segreduce_reference import ACC, bits, from_acc, same_bits, store, to_acc  # noqa: F401

FLOATS = ('f32', 'f64', 'f16', 'bf16')
CODE = {'f32': 0, 'f64': 1, 'f16': 2, 'bf16': 3}
ITEM = {'f32': 4, 'f64': 8, 'f16': 2, 'bf16': 2}
U = {'f32': 2.0 ** -24, 'f16': 2.0 ** -24, 'bf16': 2.0 ** -24, 'f64': 2.0 ** -53}  # unit roundoff of the accumulator
SUBNORMAL = {'f32': 2.0 ** -149, 'f16': 2.0 ** -149, 'bf16': 2.0 ** -149, 'f64': 2.0 ** -1074}
SDDMM_MUTANTS = ('head_leak', 'scale_twice', 'perm_ignored')
SPMM_MUTANTS = ('tail_dropped', 'perm_on_ind', 'empty_not_zeroed', 'head_tail_swapped', 'acc_not_cleared',
                'value_of_next_head')
LD = np.longdouble  # the oracles add in extended precision where the platform has it

Case = namedtuple('Case', 'name ptr ind E nseg nsrc')
SdRoute = namedtuple('SdRoute', 'generic vec lanes_per_head side_by_side heads_per_pass window block max_heads')
ShRoute = namedtuple('ShRoute', 'generic vec lanes_per_row groups chunk tile staged blocks')


def _fake(aligned):
    return ctypes.c_void_p(0x1000 if aligned else 0x1008)  # never dereferenced


def sddmm_route(dtype, H, D, aligned=True):
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_sddmm_heads_route(CODE[dtype], H, D, _fake(aligned), _fake(aligned), out) == 0
    return SdRoute(*[int(v) for v in out])


def spmm_route(dtype, H, D, aligned=True):
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spmm_heads_route(CODE[dtype], H, D, _fake(aligned), _fake(aligned), out) == 0
    return ShRoute(*[int(v) for v in out])


def expected_sddmm_route(dtype, H, D, aligned):
    """What the header documents, restated: 0 packets, 1 generic."""
    vec = 16 // ITEM[dtype]
    packets = D % vec == 0 and aligned and (D // vec) & (D // vec - 1) == 0
    return 0 if packets else 1


def expected_spmm_route(dtype, H, D, aligned):
    return 0 if D % (16 // ITEM[dtype]) == 0 and aligned else 1


# ---- oracles: loops over the entries -----------------------------------------------------------------------------
def _seg_of(ptr, nseg, E):
    ptr = np.asarray(ptr, np.int64)[:nseg + 1]
    assert E == 0 or (ptr[0] == 0 and int(ptr[-1]) == E and bool((np.diff(ptr) >= 0).all()))
    return np.repeat(np.arange(nseg, dtype=np.int64), np.diff(ptr)) if nseg else np.zeros(0, np.int64)


def _order(perm, E):
    return np.arange(E, dtype=np.int64) if perm is None else np.asarray(perm, np.int64)


def sddmm_exact(ptr, ind, perm, q, k, scale=1.0):
    """q [nseg, H, D], k [nsrc, H, D] numbers -> (out64 [E, H], sum|terms| [E, H], terms per output = D); entry i of the
    segmented order is element perm[i] of the result."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    E, H, D = len(ind), q.shape[1], q.shape[2]
    seg, p = _seg_of(ptr, q.shape[0], E), _order(perm, E)
    out, mass = np.zeros((E, H)), np.zeros((E, H))
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(E):
            t = LD(scale) * q[seg[i]].astype(LD) * k[ind[i]].astype(LD)
            out[p[i]] = t.sum(-1)
            mass[p[i]] = np.abs(t).sum(-1)
    return out, mass, D


def spmm_exact(ptr, ind, perm, value, x, nseg):
    """value [E, H] numbers or None, x [nsrc, H, D] -> (out64 [nseg, H, D], sum|terms|, terms per output [nseg, 1, 1] =
    2 * segment length: a product and its rounding)."""
    x = np.asarray(x, np.float64)
    E, H, D = len(ind), x.shape[1], x.shape[2]
    v = np.ones((E, H)) if value is None else np.asarray(value, np.float64)
    seg, p = _seg_of(ptr, nseg, E), _order(perm, E)
    out, mass = np.zeros((nseg, H, D), LD), np.zeros((nseg, H, D), LD)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(E):
            t = v[p[i]].astype(LD)[:, None] * x[ind[i]].astype(LD)
            out[seg[i]] += t
            mass[seg[i]] += np.abs(t)
    n = 2 * np.diff(np.asarray(ptr, np.int64)[:nseg + 1]).reshape(nseg, 1, 1)
    return out.astype(np.float64), mass.astype(np.float64), n


def sddmm_grads_exact(rowptr, col, q, k, scale, g):
    """Gradients of sum(g * sddmm(q, k, scale)): -> ((grad_q, mass, n), (grad_k, mass, n))."""
    q, k, g = np.asarray(q, np.float64), np.asarray(k, np.float64), np.asarray(g, np.float64)
    E = len(col)
    row = _seg_of(rowptr, q.shape[0], E)
    gq, mq, gk, mk = [np.zeros(a.shape, LD) for a in (q, q, k, k)]
    for e in range(E):
        w = (LD(scale) * g[e].astype(LD))[:, None]
        tq, tk = w * k[col[e]].astype(LD), w * q[row[e]].astype(LD)
        gq[row[e]] += tq
        mq[row[e]] += np.abs(tq)
        gk[col[e]] += tk
        mk[col[e]] += np.abs(tk)
    nq = 2 * np.bincount(row, minlength=q.shape[0]).reshape(-1, 1, 1) + 1  # + 1: the multiplication by scale
    nk = 2 * np.bincount(col, minlength=k.shape[0]).reshape(-1, 1, 1) + 1
    f = np.float64
    return (gq.astype(f), mq.astype(f), nq), (gk.astype(f), mk.astype(f), nk)


def spmm_grads_exact(rowptr, col, value, x, nseg, go):
    """Gradients of sum(go * spmm(value, x)): -> ((grad_value [E, H], mass, n = D), (grad_x, mass, n))."""
    v, x, go = np.asarray(value, np.float64), np.asarray(x, np.float64), np.asarray(go, np.float64)
    E = len(col)
    row = _seg_of(rowptr, nseg, E)
    gv, mv = np.zeros(v.shape), np.zeros(v.shape)
    gx, mx = np.zeros(x.shape, LD), np.zeros(x.shape, LD)
    for e in range(E):
        t = go[row[e]].astype(LD) * x[col[e]].astype(LD)
        gv[e] = t.sum(-1)
        mv[e] = np.abs(t).sum(-1)
        tx = v[e].astype(LD)[:, None] * go[row[e]].astype(LD)
        gx[col[e]] += tx
        mx[col[e]] += np.abs(tx)
    nx = 2 * np.bincount(col, minlength=x.shape[0]).reshape(-1, 1, 1)
    return (gv, mv, x.shape[2]), (gx.astype(np.float64), mx.astype(np.float64), nx)


def csc_of(case):
    """(colptr, row ids in column order, csr2csc) of a case, by a stable sort."""
    row = _seg_of(case.ptr, case.nseg, case.E)
    csr2csc = np.argsort(case.ind, kind='stable').astype(np.int64)
    colptr = np.zeros(case.nsrc + 1, np.int64)
    np.cumsum(np.bincount(case.ind, minlength=case.nsrc), out=colptr[1:])
    return colptr, row[csr2csc], csr2csc


# ---- comparators -------------------------------------------------------------------------------------------------
def _half_ulp(x, dtype):
    """Half an ulp of |x| in a 16-bit storage type (0 for f32 / f64: the bound's u covers their store)."""
    if dtype == 'f16':
        with np.errstate(over='ignore', invalid='ignore'):
            return 0.5 * np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)
    if dtype == 'bf16':
        with np.errstate(divide='ignore', invalid='ignore'):
            e = np.floor(np.log2(np.abs(x)))
        return 0.5 * np.exp2(np.maximum(np.where(np.isfinite(e), e, -126.0), -126.0) - 7)
    return np.zeros_like(x)


def bound_of(ref, mass, n, dtype):
    with np.errstate(invalid='ignore'):
        b = (n + 2) * U[dtype] * mass + n * SUBNORMAL[dtype]
        return b + _half_ulp(np.abs(ref) + b, dtype)


def check(got, expect, dtype):
    """got: stored elements; expect = (ref64, sum|terms|, n).  Non-finite exactly where and as the oracle has it,
    elsewhere inside bound_of.  -> the worst error / bound."""
    ref, mass, n = expect
    g = to_acc(got, dtype).astype(np.float64)
    assert g.shape == ref.shape, 'shape %s, expected %s' % (g.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(g), nan), '%s: %d NaN positions differ' % (dtype, int((np.isnan(g) != nan).sum()))
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(g), inf) and bool((g[inf] == ref[inf]).all()), '%s: infinities differ' % dtype
    ok = ~nan & ~inf
    bound = bound_of(ref, mass, n * np.ones_like(ref), dtype)
    err = np.abs(g - ref)
    zero = ok & (bound == 0)
    assert bool((err[zero] == 0).all()), '%s: an exact zero is not zero' % dtype
    ok &= bound > 0
    ratio = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    assert ratio <= 1.0, '%s: worst error / bound %.3g at %s' % (
        dtype, ratio, np.unravel_index(np.argmax(np.where(ok, err / np.where(ok, bound, 1), 0)), ref.shape))
    return ratio


def rejects(got, expect, dtype):
    try:
        check(got, expect, dtype)
    except AssertionError:
        return True
    return False


# ---- layouts -----------------------------------------------------------------------------------------------------
def _case(name, lens, nsrc, rng):
    lens = np.asarray(lens, np.int64)
    ptr = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    E = int(ptr[-1])
    return Case(name, ptr, rng.integers(0, nsrc, E).astype(np.int64), E, int(lens.size), nsrc)


def _short_rows(rng, total):
    """Row lengths 0..7 that add up to `total`."""
    lens = []
    while total > 0:
        n = min(int(rng.integers(0, 8)), total)
        lens.append(n)
        total -= n
    return lens


def edge_sizes(chunk, window, block, tile):
    """E = 1 and every tile edge of both kernels, minus one, exact, plus one."""
    sizes = {1}
    for s in (chunk, window, block, tile):
        sizes.update((s - 1, s, s + 1))
    return sorted(x for x in sizes if x >= 1)


def edge_case(E, nsrc=37, seed=3):
    rng = np.random.default_rng(seed + E)
    return _case('edge_%d' % E, _short_rows(rng, E), nsrc, rng)


def hub_case(chunk, tile, nsrc=53, seed=4):
    """Two empty leading rows, a row of one, a hub of 3 * chunk + 5 entries beside rows of length 0 and 1, short rows up
    to past the next tile boundary, a row cut by exactly one chunk boundary, three empty trailing rows."""
    rng = np.random.default_rng(seed)
    lens = [0, 0, 1, 3 * chunk + 5, 0, 1]
    used = sum(lens)
    fill = _short_rows(rng, (-used) % chunk + chunk - 3)  # stop 3 short of a chunk boundary ...
    lens += fill + [7]                                    # ... so this row is cut once
    lens += _short_rows(rng, max(tile + 9 - sum(lens), 5)) + [0, 0, 0]
    return _case('hub', lens, nsrc, rng)


def one_source_case(chunk, seed=5):
    rng = np.random.default_rng(seed)
    return _case('one_source', _short_rows(rng, chunk + 11) + [0], 1, rng)


def sparse_rows_case(staged, seed=6):
    """More segments inside one tile than its LDS slice holds: the pointer search goes to global memory."""
    rng = np.random.default_rng(seed)
    return _case('sparse_rows', [2, 1] + [0] * (staged + 40) + [3] + [0] * 5 + [1, 4], 11, rng)


def census(case, chunk, tile, staged):
    """What the rows of a layout meet: {'empty', 'inside' (one chunk), 'cut' (two chunks), 'span3' (three or more)} ->
    row counts, plus 'unstaged': tiles that meet more than `staged` segments."""
    out = {'empty': 0, 'inside': 0, 'cut': 0, 'span3': 0, 'unstaged': 0}
    for s in range(case.nseg):
        a, b = int(case.ptr[s]), int(case.ptr[s + 1])
        if a == b:
            out['empty'] += 1
            continue
        chunks = (b - 1) // chunk - a // chunk + 1
        out['inside' if chunks == 1 else 'cut' if chunks == 2 else 'span3'] += 1
    seg = _seg_of(case.ptr, case.nseg, case.E)
    for e0 in range(0, case.E, tile):
        e1 = min(e0 + tile, case.E)
        out['unstaged'] += int(seg[e1 - 1] - seg[e0] + 1 > staged)
    return out


def assert_census(dtype, H, D):
    """The layouts of (dtype, H, D) reach what they are built for -> the cases."""
    r = spmm_route(dtype, H, D)
    assert r.chunk == 8 * r.lanes_per_row and r.groups * r.lanes_per_row == 64 and r.tile == 2048, r
    hub, rare = hub_case(r.chunk, r.tile), sparse_rows_case(r.staged)
    c = census(hub, r.chunk, r.tile, r.staged)
    assert c['empty'] >= 6 and c['inside'] >= 3 and c['cut'] >= 1 and c['span3'] >= 1 and c['unstaged'] == 0, c
    assert hub.E > r.tile and int(np.diff(hub.ptr).max()) >= 3 * r.chunk
    assert census(rare, r.chunk, r.tile, r.staged)['unstaged'] == 1
    return [hub, rare, one_source_case(r.chunk)]


def operands(case, dtype, H, D, seed=0, with_value=True):
    """(q [nseg, H, D], k [nsrc, H, D], value [E, H]) as stored elements of `dtype`."""
    rng = np.random.default_rng(seed)
    q = store(rng.standard_normal((case.nseg, H, D)), dtype)
    k = store(rng.standard_normal((case.nsrc, H, D)), dtype)
    v = store(rng.standard_normal((case.E, H)), dtype) if with_value else None
    return q, k, v


def numbers(a, dtype):
    return None if a is None else to_acc(a, dtype).astype(np.float64)


# ---- the kernels by pieces, with planted defects -------------------------------------------------------------------
def emulate_sddmm(ptr, ind, perm, q, k, scale, lanes_per_head, vec, mutant=None):
    """csrc/sddmm.hip in fp64: lane l of a head adds packets l, l + LPH, ... of `vec` features, a xor butterfly over the
    LPH lanes, scale on the result, stored at perm[i]."""
    assert mutant is None or mutant in SDDMM_MUTANTS
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    E, H, D = len(ind), q.shape[1], q.shape[2]
    seg, p = _seg_of(ptr, q.shape[0], E), _order(perm, E)
    out = np.zeros((E, H))
    slots = -(-D // vec)
    for i in range(E):
        lanes = np.zeros((H, lanes_per_head))
        for h in range(H):
            for l in range(lanes_per_head):
                for s in range(l, slots, lanes_per_head):
                    d = slice(s * vec, min((s + 1) * vec, D))
                    lanes[h, l] += float((q[seg[i], h, d] * k[ind[i], h, d]).sum())
        flat = lanes.reshape(-1)
        width = lanes_per_head * (2 if mutant == 'head_leak' and H > 1 else 1)  # the butterfly one step too far
        for h in range(H):
            lo = (h * lanes_per_head) // width * width
            acc = flat[lo:lo + width].sum() * scale
            if mutant == 'scale_twice':
                acc *= scale
            out[i if mutant == 'perm_ignored' else p[i], h] = acc
    return out


def emulate_spmm(ptr, ind, perm, value, x, nseg, chunk, mutant=None):
    """csrc/spmm_heads.hip in fp64: every chunk of `chunk` entries walks its entries in order; a segment that ends in
    the chunk is written, or left as the HEAD record when it began before the chunk; what is open at the end is the
    TAIL record; the fix-up adds the tail records of [ptr[s] // chunk, b) in order, then the head record."""
    assert mutant is None or mutant in SPMM_MUTANTS
    x = np.asarray(x, np.float64)
    ind = np.asarray(ind, np.int64)
    E, H, D = len(ind), x.shape[1], x.shape[2]
    v = np.ones((E, H)) if value is None else np.asarray(value, np.float64)
    ptr = np.asarray(ptr, np.int64)
    seg, p = _seg_of(ptr, nseg, E), _order(perm, E)
    out = np.full((nseg, H, D), 85.0 if mutant == 'empty_not_zeroed' else 0.0)  # the memset
    nchunks = -(-E // chunk)
    head = [None] * nchunks
    tail = [None] * nchunks
    for c in range(nchunks):
        c0, c1 = c * chunk, min((c + 1) * chunk, E)
        acc = np.zeros((H, D))
        is_open = False
        for i in range(c0, c1):
            s = seg[i]
            w = v[p[i]]
            if mutant == 'value_of_next_head':
                w = np.roll(w, -1)
            src = ind[p[i]] if mutant == 'perm_on_ind' else ind[i]
            if mutant == 'perm_on_ind':
                w = v[i]
            acc = acc + w[:, None] * x[src]
            is_open = True
            if i + 1 == ptr[s + 1]:
                if ptr[s] >= c0:
                    out[s] = acc
                else:
                    head[c] = (s, acc)
                if mutant != 'acc_not_cleared':
                    acc = np.zeros((H, D))
                is_open = False
        if is_open:
            tail[c] = (seg[c1 - 1], acc)
    for b in range(nchunks):
        if head[b] is None:
            continue
        s, hv = head[b]
        first = int(ptr[s]) // chunk
        pieces = [tail[i][1] for i in range(first, b - 1 if mutant == 'tail_dropped' else b)]
        if mutant == 'head_tail_swapped' and tail[b] is not None:
            hv = tail[b][1]  # the record of the segment that BEGINS in the chunk
        total = np.zeros((H, D))
        for t in pieces:
            total = total + t
        out[s] = total + hv
    return out
