"""Reference of the fused attention (csrc/attention.hip): an fp64 oracle of the forward (out, lse) and of everything the
backward computes (p, ds, the four gradients) written as loops over the rows and their entries, the comparators with a
derived bound, layouts sized from tsamd_attention_heads_route with a host census, and a numpy restatement of the chunk /
record / fix-up scheme with the online combine whose switches plant defects.  numpy only (ctypes for the route).

Element types are named 'f32' 'f64' 'f16' 'bf16'; a bf16 array is carried as its uint16 bits (tests/util.py).

The bound (derived in docs/design/widening.md, "Fused attention").  u is the unit roundoff of the accumulator.  The kernel's
weight of entry i is e(s_i - m_1) * prod_j e(m_j - m_{j+1}) over the changes of the running maximum that follow it, the
exact one exp(s_i - m).  Its relative error eta_i is at most
    (D + 3) u mass_i             the computed score: mass_i = |scale| sum_d |q k| + |bias_i| (attention_reference.bound_of
                                 for the dot product and the scale, one more rounding for the bias)
  + 2 |s_i - m| u                the arguments of e: they telescope to s_i - m, all of one sign; __expf multiplies the
                                 argument by log2(e) (one rounding) before the hardware exp2, exp is as good
  + 5 (n + 1) u                  per factor: e's own error (2 ulp), the subtraction and the multiplication; at most one
                                 factor per change of the maximum, at most the row length n.
With out = sum w_i v_i / sum w_i,  |d out| <= sum p_i eta_i (|v_i| + |out|) + (2 n + 2) u sum p_i |v_i| (the n u of the two
sums, the division) + half an ulp of the stored type + n * tiny.  lse = m + log(l) moves by at most sum p_i eta_i +
(n + 2) u + 3 u (|m| + |log l|) + u |lse|."""
import ctypes
from collections import namedtuple

import numpy as np

from pytorch_sparse_amd import _native as nat
from tests import attention_reference as AR
from tests.attention_reference import (CODE, FLOATS, ITEM, LD, SUBNORMAL, U, Case, _half_ulp, _seg_of, census,  # noqa: F401
                                       edge_case, edge_sizes, hub_case, numbers, one_source_case, sparse_rows_case)
from tests.segreduce_reference import ACC, same_bits, store, to_acc  # noqa: F401

MUTANTS = ('no_rescale_on_new_max', 'tail_dropped', 'head_tail_swapped', 'state_not_cleared_at_row_end',
           'max_shared_between_heads', 'scale_after_bias', 'lse_without_max', 'empty_row_not_zero',
           'bias_of_next_entry')
PEAKS = ('first', 'last', 'both')

AtRoute = namedtuple('AtRoute', 'generic vec lanes_per_head heads_per_pass blocks chunk tile fblocks')
Expect = namedtuple('Expect', 'out lse n pav a1 a2 b1 b2 m logl p s mass')


def route(dtype, H, D, aligned=True):
    out = (ctypes.c_int64 * 8)()
    f = AR._fake(aligned)
    assert nat.lib().tsamd_attention_heads_route(CODE[dtype], H, D, f, f, f, f, out) == 0
    return AtRoute(*[int(v) for v in out])


def expected_route(dtype, H, D, aligned):
    """What the header documents, restated -> (generic, vec, lanes per head, heads per pass, blocks, chunk, 2048, fblocks)."""
    vec = 16 // ITEM[dtype]
    packets = D % vec == 0 and aligned
    slots = -(-D // vec)
    lph = 1
    while lph < min(slots, 64):
        lph *= 2
    hpp = 1
    while hpp < H and hpp * lph < 64:
        hpp *= 2
    fblocks = -(-slots // 64)
    return AtRoute(0 if packets else 1, vec if packets else 1, lph, hpp, -(-H // hpp) * fblocks, 8 * lph * hpp, 2048, fblocks)


def workspace_bytes(dtype, H, D, E):
    """The formula of the header."""
    acc = 8 if dtype == 'f64' else 4
    r = expected_route(dtype, H, D, True)
    nchunks = -(-max(E, 1) // r.chunk)
    up = lambda x: -(-x // 256) * 256  # noqa: E731
    return 2 * up(acc * nchunks * H * D) + 2 * up(2 * acc * nchunks * H) + 2 * up(8 * nchunks)


# ---- oracle --------------------------------------------------------------------------------------------------------
def _bias_rows(bias, E, H):
    if bias is None:
        return np.zeros((E, H))
    b = np.asarray(bias, np.float64)
    return np.repeat(b[:, None], H, 1) if b.ndim == 1 else b


def exact(ptr, ind, bias, q, k, v, scale):
    """q [M, H, D], k, v [N, H, D] numbers, bias None / [E] / [E, H] -> Expect.  Per row and head: m = max s,
    p = exp(s - m) / sum; a NaN or +inf score or a row of -inf only makes out NaN (lse NaN, -inf for the row of -inf)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    ptr, ind = np.asarray(ptr, np.int64), np.asarray(ind, np.int64)
    M, H, D = q.shape
    E = len(ind)
    b = _bias_rows(bias, E, H)
    out, pav, a1, a2 = (np.zeros((M, H, D)) for _ in range(4))
    lse = np.full((M, H), -np.inf)
    b1, b2, m_, logl = (np.zeros((M, H)) for _ in range(4))
    p_all, s_all, mass_all = (np.zeros((E, H)) for _ in range(3))
    n = np.diff(ptr[:M + 1])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for r in range(M):
            lo, hi = int(ptr[r]), int(ptr[r + 1])
            if lo == hi:
                continue
            kk, vv = k[ind[lo:hi]], v[ind[lo:hi]]                      # [n, H, D]
            t = LD(scale) * q[r].astype(LD)[None] * kk.astype(LD)
            s = (t.sum(-1) + b[lo:hi].astype(LD)).astype(np.float64)   # [n, H]
            mass = np.abs(t).sum(-1).astype(np.float64) + np.abs(b[lo:hi])
            m = s.max(0)
            ex = np.exp((s - m).astype(LD))
            l = ex.sum(0)
            p = (ex / l).astype(np.float64)
            bad = ~np.isfinite(m) | np.isnan(s).any(0)
            p[:, bad] = np.nan
            o = (p.astype(LD)[:, :, None] * vv.astype(LD)).sum(0).astype(np.float64)
            av = (p[:, :, None] * np.abs(vv)).sum(0)
            w = np.abs(vv) + np.abs(o)[None]
            dist = np.abs(s - m)
            dist[~np.isfinite(dist)] = 0.0  # a masked entry weighs exactly zero
            out[r], pav[r] = o, av
            a1[r] = (p[:, :, None] * mass[:, :, None] * w).sum(0)
            a2[r] = (p[:, :, None] * dist[:, :, None] * w).sum(0)
            b1[r], b2[r] = (p * mass).sum(0), (p * dist).sum(0)
            m_[r], logl[r] = m, np.log(l).astype(np.float64)
            lse[r] = np.where(bad, np.where(np.isneginf(s).all(0), -np.inf, np.nan), m + logl[r])
            p_all[lo:hi], s_all[lo:hi], mass_all[lo:hi] = p, s, mass
    return Expect(out, lse, n, pav, a1, a2, b1, b2, m_, logl, p_all, s_all, mass_all)


def bounds(ex, D, dtype):
    """-> (bound of out [M, H, D], bound of lse [M, H])."""
    u = U[dtype]
    n = ex.n.astype(np.float64)
    n3, n2 = n[:, None, None], n[:, None]
    with np.errstate(invalid='ignore'):
        bo = u * ((D + 3) * ex.a1 + 2 * ex.a2 + (5 * n3 + 5) * (ex.pav + np.abs(ex.out)) + (2 * n3 + 2) * ex.pav)
        bo = bo + n3 * SUBNORMAL[dtype]
        bo = bo + _half_ulp(np.abs(ex.out) + bo, dtype)
        bl = u * ((D + 3) * ex.b1 + 2 * ex.b2 + (5 * n2 + 5) + (n2 + 2) + 3 * (np.abs(ex.m) + np.abs(ex.logl)) +
                  np.abs(ex.lse))
    return bo, bl


def _ratio(g, ref, bound, what, dtype):
    assert g.shape == ref.shape, '%s: shape %s, expected %s' % (what, g.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(g), nan), '%s %s: %d NaN positions differ' % (dtype, what, int((np.isnan(g) != nan).sum()))
    inf = np.isinf(ref)
    assert np.array_equal(np.isinf(g), inf) and bool((g[inf] == ref[inf]).all()), '%s %s: infinities differ' % (dtype, what)
    ok = ~nan & ~inf
    err = np.abs(np.where(ok, g - np.where(ok, ref, 0), 0))
    zero = ok & (bound == 0)
    assert bool((err[zero] == 0).all()), '%s %s: an exact zero is not zero' % (dtype, what)
    ok &= bound > 0
    if not ok.any():
        return 0.0
    rel = np.where(ok, err / np.where(ok, bound, 1), 0)
    ratio = float(rel.max())
    assert ratio <= 1.0, '%s %s: worst error / bound %.3g at %s' % (dtype, what, ratio,
                                                                     np.unravel_index(np.argmax(rel), ref.shape))
    return ratio


def check(got_out, got_lse, ex, dtype):
    """got_out: stored elements [M, H, D]; got_lse: accumulator numbers [M, H].  Non-finite exactly where and as the
    oracle has it, rows without entries exactly zero / -inf, elsewhere inside the bound -> (ratio of out, ratio of lse)."""
    D = ex.out.shape[2]
    bo, bl = bounds(ex, D, dtype)
    g = to_acc(got_out, dtype).astype(np.float64)
    return (_ratio(g, ex.out, bo, 'out', dtype),
            _ratio(np.asarray(got_lse, np.float64), ex.lse, bl, 'lse', dtype))


def rejects(got_out, got_lse, ex, dtype):
    try:
        check(got_out, got_lse, ex, dtype)
    except AssertionError:
        return True
    return False


def bw_exact(ptr, ind, bias, q, k, v, out, lse, go, scale):
    """What tsamd_attention_heads_bw computes FROM THE GIVEN out and lse: -> (p [E, H], ds [E, H], bound of p, bound of ds
    without the unit roundoff: multiply by u)."""
    q, k, v, out, lse, go = (np.asarray(a, np.float64) for a in (q, k, v, out, lse, go))
    M, H, D = q.shape
    E = len(ind)
    row = _seg_of(ptr, M, E)
    b = _bias_rows(bias, E, H)
    with np.errstate(invalid='ignore', over='ignore'):
        t = LD(scale) * q[row].astype(LD) * k[ind].astype(LD)
        s = (t.sum(-1) + b).astype(np.float64)
        mass = np.abs(t).sum(-1).astype(np.float64) + np.abs(b)
        dp = (go[row].astype(LD) * v[ind].astype(LD)).sum(-1).astype(np.float64)
        dl = (go[row].astype(LD) * out[row].astype(LD)).sum(-1).astype(np.float64)
        mdp = (np.abs(go[row] * v[ind])).sum(-1) + (np.abs(go[row] * out[row])).sum(-1)
        ls = lse[row]
        p = np.exp(s - ls)
        ds = p * (dp - dl)
        dead = ~np.isfinite(ls)
        p[dead], ds[dead] = np.nan, np.nan
        masked = np.isneginf(s) & ~dead
        p[masked], ds[masked] = 0.0, 0.0
        dist = np.abs(np.where(np.isfinite(s - ls), s - ls, 0.0))
        rel = (D + 3) * mass + np.abs(ls) + 2 * dist + 6      # of p, in units of u
        bp = p * rel
        bd = np.abs(ds) * (rel + 2) + p * (D + 3) * mdp
    return p, ds, bp, bd


def check_bw(got_p, got_ds, expect, dtype):
    p, ds, bp, bd = expect
    u = U[dtype]
    out = []
    for got, ref, b, what in ((got_p, p, bp, 'p'), (got_ds, ds, bd, 'ds')):
        bound = u * b + SUBNORMAL[dtype] * (ref != 0)
        bound = np.where(np.isfinite(bound), bound + _half_ulp(np.abs(ref) + bound, dtype) * (ref != 0), bound)
        out.append(_ratio(to_acc(got, dtype).astype(np.float64), ref, bound, what, dtype))
    return tuple(out)


def grads_exact(ptr, ind, bias, q, k, v, scale, go):
    """fp64 gradients of sum(go * attention(q, k, v)) -> (grad_q, grad_k, grad_v, grad_bias [E, H]), loops over the rows."""
    q, k, v, go = (np.asarray(a, np.float64) for a in (q, k, v, go))
    ex = exact(ptr, ind, bias, q, k, v, scale)
    M, H, D = q.shape
    gq, gk, gv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    ds = np.zeros((len(ind), H))
    for r in range(M):
        for e in range(int(ptr[r]), int(ptr[r + 1])):
            c = ind[e]
            p = ex.p[e]
            dp = (go[r] * v[c]).sum(-1)
            dl = (go[r] * ex.out[r]).sum(-1)
            ds[e] = p * (dp - dl)
            gq[r] += scale * ds[e][:, None] * k[c]
            gk[c] += scale * ds[e][:, None] * q[r]
            gv[c] += p[:, None] * go[r]
    return gq, gk, gv, ds


# ---- layouts and operands ------------------------------------------------------------------------------------------
def layouts(dtype, H, D):
    """The census layouts of (dtype, H, D), sized from the route query -> (route, [hub, sparse_rows, one_source])."""
    r = route(dtype, H, D)
    assert r.chunk == 8 * r.lanes_per_head * r.heads_per_pass and r.tile == 2048, r
    hub, rare = hub_case(r.chunk, r.tile), sparse_rows_case(r.tile)
    c = census(hub, r.chunk, r.tile, r.tile)
    assert c['empty'] >= 6 and c['inside'] >= 3 and c['cut'] >= 1 and c['span3'] >= 1 and c['unstaged'] == 0, c
    assert hub.E > r.tile and int(np.diff(hub.ptr).max()) == 3 * r.chunk + 5
    assert hub.ptr[1] == 0 and hub.ptr[-1] == hub.ptr[-4], 'empty leading and trailing rows'
    assert census(rare, r.chunk, r.tile, r.tile)['unstaged'] == 1
    one = one_source_case(r.chunk)
    assert one.nsrc == 1
    return r, [hub, rare, one]


def peak_bias(case, chunk, where, height=12.0, seed=7):
    """A [nnz] bias that puts the largest score of the hub row into its first chunk, its last chunk, or -- the same
    maximum -- into both; small elsewhere."""
    assert where in PEAKS
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(case.E) * 0.25
    hub = int(np.argmax(np.diff(case.ptr)))
    lo, hi = int(case.ptr[hub]), int(case.ptr[hub + 1])
    assert (hi - 1) // chunk - lo // chunk >= 3
    if where in ('first', 'both'):
        b[lo + 1] = height
    if where in ('last', 'both'):
        b[hi - 2] = height
    return b


def operands(case, dtype, H, D, seed=0, spread=1.0):
    """(q [nseg, H, D], k [nsrc, H, D], v [nsrc, H, D]) as stored elements; spread scales q: with spread * scale * sqrt(D)
    near 80 the scores reach +-80, where an unshifted fp32 exp overflows or flushes."""
    rng = np.random.default_rng(seed)
    q = store(rng.standard_normal((case.nseg, H, D)) * spread, dtype)
    k = store(rng.standard_normal((case.nsrc, H, D)), dtype)
    v = store(rng.standard_normal((case.nsrc, H, D)), dtype)
    return q, k, v


def composition_f32(ptr, ind, bias, q, k, v, scale):
    """The three steps in float32 torch on the CPU, row by row: scores, torch.softmax, weighted sum -> (out, lse)."""
    import torch
    q, k, v = (torch.from_numpy(np.asarray(a, np.float32)) for a in (q, k, v))
    M, H, D = q.shape
    b = None if bias is None else torch.from_numpy(_bias_rows(bias, len(ind), H).astype(np.float32))
    out, lse = torch.zeros(M, H, D), torch.full((M, H), -np.inf)
    col = torch.from_numpy(np.asarray(ind, np.int64))
    for r in range(M):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        if lo == hi:
            continue
        s = (q[r][None] * k[col[lo:hi]]).sum(-1) * np.float32(scale)
        if b is not None:
            s = s + b[lo:hi]
        out[r] = (torch.softmax(s, 0)[:, :, None] * v[col[lo:hi]]).sum(0)
        lse[r] = torch.logsumexp(s, 0)
    return out.numpy(), lse.numpy()


# ---- the kernel by pieces, with planted defects ---------------------------------------------------------------------
def _e(x):
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return np.exp(x)


def _combine(m, l, a, m2, l2, a2, rescale=True):
    """(m, l, a) (+) (m2, l2, a2) per head, in the dtype of the operands: the combine of csrc/softmax.hip with an
    accumulator row."""
    with np.errstate(invalid='ignore', over='ignore'):
        first = m >= m2
        hi, lo = np.where(first, m, m2), np.where(first, m2, m)
        f = np.where(np.isneginf(lo), lo.dtype.type(0), _e(lo - hi))
        one = lo.dtype.type(1)
        fa, fb = np.where(first, one, f), np.where(first, f, one)
        if not rescale:
            fa = np.where(first, one, one)
        return hi, l * fa + l2 * fb, a * fa[:, None] + a2 * fb[:, None]


def _final(m, l, a, with_max=True):
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        lf = np.where(m < np.inf, l, np.nan).astype(l.dtype)
        return a / lf[:, None], (m if with_max else 0) + np.log(lf)


def emulate(ptr, ind, bias, q, k, v, scale, chunk, dtype, mutant=None):
    """csrc/attention.hip in the accumulator type of `dtype`: the fill, every chunk of `chunk` entries walked in order
    with the online update per head, rows that end in their chunk written, head / tail records for the cut ones, the
    fix-up folding tails [ptr[s] // chunk, b) and the head record.  q, k, v, bias: numbers.  -> (out, lse) in the
    accumulator type."""
    assert mutant is None or mutant in MUTANTS
    A = ACC[dtype]
    q, k, v = (np.asarray(a).astype(A) for a in (q, k, v))
    ptr, ind = np.asarray(ptr, np.int64), np.asarray(ind, np.int64)
    M, H, D = q.shape
    E = len(ind)
    b = _bias_rows(bias, E, H).astype(A)
    seg = _seg_of(ptr, M, E)
    out = np.full((M, H, D), 85.0 if mutant == 'empty_row_not_zero' else 0.0, A)
    lse = np.full((M, H), -np.inf, A)
    nchunks = -(-E // chunk)
    head, tail = [None] * nchunks, [None] * nchunks
    fresh = lambda: (np.full(H, -np.inf, A), np.zeros(H, A), np.zeros((H, D), A))  # noqa: E731
    sc = A(scale)
    with_max = mutant != 'lse_without_max'
    for c in range(nchunks):
        c0, c1 = c * chunk, min((c + 1) * chunk, E)
        m, l, acc = fresh()
        is_open = False
        for i in range(c0, c1):
            r = seg[i]
            bi = b[min(i + 1, E - 1)] if mutant == 'bias_of_next_entry' else b[i]
            dot = (q[r] * k[ind[i]]).sum(-1, dtype=A)
            with np.errstate(invalid='ignore', over='ignore'):
                s = (dot + bi) * sc if mutant == 'scale_after_bias' else dot * sc + bi
            if mutant == 'max_shared_between_heads':
                with np.errstate(invalid='ignore'):
                    top = np.full(H, max(float(m.max()), float(s.max())), A)
                f_old = np.where(np.isneginf(m), A(0), _e(m - top))
                f_new = np.where(np.isneginf(s), A(0), _e(s - top))
                m, l, acc = top, l * f_old + f_new, acc * f_old[:, None] + f_new[:, None] * v[ind[i]]
            else:
                m, l, acc = _combine(m, l, acc, s, np.ones(H, A), v[ind[i]], rescale=mutant != 'no_rescale_on_new_max')
            is_open = True
            if i + 1 == ptr[r + 1]:
                if ptr[r] >= c0:
                    out[r], lse[r] = _final(m, l, acc, with_max)
                else:
                    head[c] = (r, (m, l, acc))
                if mutant != 'state_not_cleared_at_row_end':
                    m, l, acc = fresh()
                is_open = False
        if is_open:
            tail[c] = (seg[c1 - 1], (m, l, acc))
    for bq in range(nchunks):
        if head[bq] is None:
            continue
        r, hv = head[bq]
        first = int(ptr[r]) // chunk
        pieces = [tail[i][1] for i in range(first, bq - 1 if mutant == 'tail_dropped' else bq)]
        if mutant == 'head_tail_swapped' and tail[bq] is not None:
            hv = tail[bq][1]  # the record of the row that BEGINS in the chunk
        m, l, acc = fresh()
        for t in pieces + [hv]:
            m, l, acc = _combine(m, l, acc, *t)
        out[r], lse[r] = _final(m, l, acc, with_max)
    return out, lse
