"""Reference of dropout on the probabilities of the fused attention calls (csrc/attention.hip, DROP instantiations), for
both score modes: the mask restated from oracle/np_draws.philox, an fp64 oracle of the forward and of everything the
backward computes, comparators with a derived bound, and a numpy restatement of the chunk / record scheme with dropout
whose switches plant defects.  It builds on tests/fused_attention_reference.py (F) and tests/gat_attention_reference.py
(G); `mode` is 'dot' (sr, sc, scalar = q, k, scale) or 'gat' (a_dst, a_src, negative_slope).  numpy only.

The mask is a pure function of (seed, entry e in CSR storage order, head h):
    thr = floor(rate * 2^32),  r = philox(seed, e >> 2, h, 0xD20B),  keep = r[e & 3] >= thr,  c = 1 / (1 - rate)
and only the numerator of the softmax sees it: out = sum_i p_i keep_i c v_i with p the probabilities of the plain call,
lse unchanged.

The bound (derived in docs/design/widening.md, "Dropout on the probabilities") is the fused call's with pt_i = p_i
keep_i c: the kernel's weight of entry i still carries the relative error eta_i of the plain call; the accumulator row
sums pt_i v_i, so the numerator terms are weighted by pt; l sums every entry, so the denominator's relative error stays
sum p_i eta_i and multiplies |out|; c is converted to the accumulator type and multiplied into the weight: two more
roundings on every kept term,
    |d out| <= sum pt_i eta_i |v_i| + (sum p_i eta_i) |out| + (2 n + 4) u sum pt_i |v_i| + half an ulp + n * tiny.
Expect carries exactly these sums once its fields are rebuilt (exact_dropout): a1 and a2 hold the two eta terms, pav
holds sum pt_i |v_i|, and (5 n + 5) u (pav + |out|) is the per-factor part of eta with sum p_i = 1 on the |out| side."""
import math
from collections import namedtuple

import numpy as np

from oracle import np_draws as npd
from tests import fused_attention_reference as F
from tests import gat_attention_reference as G
from tests.attention_reference import LD, SUBNORMAL, U, _half_ulp, _seg_of, numbers  # noqa: F401
from tests.fused_attention_reference import _bias_rows, _ratio
from tests.segreduce_reference import ACC, store, to_acc  # noqa: F401

TAG_DROPOUT = 0xD20B
MODES = ('dot', 'gat')
FW_MUTANTS = ('mask_of_next_entry', 'mask_shared_between_heads', 'l_masked_too', 'c_missing', 'keep_inverted',
              'batch_aligned_to_window')
BW_MUTANTS = ('grad_v_uses_p', 'dp_without_keep_c')
SMALLEST_NORMAL = {'f32': 2.0 ** -126, 'f64': 2.0 ** -1022, 'f16': 2.0 ** -14, 'bf16': 2.0 ** -126}

Grads = namedtuple('Grads', 'sr sc v bias')


# ---- the mask ------------------------------------------------------------------------------------------------------
def threshold(rate):
    """floor(rate * 2^32): the product is exact in a double."""
    assert 0.0 <= rate < 1.0
    return int(math.floor(float(rate) * 4294967296.0))


def scale_of(rate):
    return 1.0 / (1.0 - float(rate))


def _words(seed, counter, h, sel):
    r = npd.philox(seed, counter, h, TAG_DROPOUT)
    return np.where(sel == 0, r[0], np.where(sel == 1, r[1], np.where(sel == 2, r[2], r[3])))


def keep_mask(seed, rate, E, H, e0=0):
    """keep [E, H] (bool) of the entries e0 .. e0 + E - 1."""
    e = (np.arange(E, dtype=np.uint64) + np.uint64(e0))[:, None]
    h = np.arange(H, dtype=np.uint64)[None, :]
    e, h = np.broadcast_arrays(e, h)
    return _words(seed, e >> np.uint64(2), h, e & np.uint64(3)) >= np.uint64(threshold(rate))


def keep_mask_by_window(seed, rate, E, H, lpr):
    """The planted defect of a group narrower than a batch that shares one Philox call all the same: the batch starts at
    the window's first entry p0 = e - e % lpr, the counter is p0 >> 2 and the word is the entry's place in the batch."""
    e = np.arange(E, dtype=np.uint64)[:, None]
    h = np.arange(H, dtype=np.uint64)[None, :]
    e, h = np.broadcast_arrays(e, h)
    p0 = e - e % np.uint64(lpr)
    return _words(seed, p0 >> np.uint64(2), h, e - p0) >= np.uint64(threshold(rate))


# ---- forward oracle ------------------------------------------------------------------------------------------------
def plain_exact(mode, ptr, ind, bias, sr, sc, v, scalar):
    """The plain call's oracle: F.exact or G.exact."""
    assert mode in MODES
    return (F.exact if mode == 'dot' else G.exact)(ptr, ind, bias, sr, sc, v, scalar)


def exact_dropout(ex, ptr, ind, v, keep, c):
    """ex: the plain oracle's Expect (p, lse, ...) -> Expect of the call with dropout: out = sum p keep c v in long double,
    and the fields the bound reads rebuilt: pav = sum pt |v|, a1 = sum pt mass |v| + (sum p mass) |out|, a2 likewise with
    |s - m|.  lse, b1, b2, m, logl, p, s and mass stay the plain call's."""
    v = np.asarray(v, np.float64)
    ptr, ind = np.asarray(ptr, np.int64), np.asarray(ind, np.int64)
    M, H, D = ex.out.shape
    with np.errstate(invalid='ignore'):
        pt_all = ex.p * (np.asarray(keep, np.float64) * c)
    out, pav, a1, a2 = (np.zeros((M, H, D)) for _ in range(4))
    with np.errstate(invalid='ignore', over='ignore'):
        for r in range(M):
            lo, hi = int(ptr[r]), int(ptr[r + 1])
            if lo == hi:
                continue
            vv = v[ind[lo:hi]]
            p, pt, mass = ex.p[lo:hi], pt_all[lo:hi], ex.mass[lo:hi]
            o = (pt.astype(LD)[:, :, None] * vv.astype(LD)).sum(0).astype(np.float64)
            dist = np.abs(ex.s[lo:hi] - ex.m[r])
            dist[~np.isfinite(dist)] = 0.0
            av = np.abs(vv)
            out[r] = o
            pav[r] = (pt[:, :, None] * av).sum(0)
            a1[r] = ((pt * mass)[:, :, None] * av).sum(0) + (p * mass).sum(0)[:, None] * np.abs(o)
            a2[r] = ((pt * dist)[:, :, None] * av).sum(0) + (p * dist).sum(0)[:, None] * np.abs(o)
    return ex._replace(out=out, pav=pav, a1=a1, a2=a2)


def bounds(mode, ex, dtype):
    """F.bounds / G.bounds on the rebuilt Expect, with (2 n + 2) -> (2 n + 4) in front of pav: c's conversion and its
    product -> (bound of out, bound of lse)."""
    u = U[dtype]
    D = ex.out.shape[2]
    ks = D + 3 if mode == 'dot' else G.KSCORE
    n3 = ex.n.astype(np.float64)[:, None, None]
    with np.errstate(invalid='ignore'):
        bo = u * (ks * ex.a1 + 2 * ex.a2 + (5 * n3 + 5) * (ex.pav + np.abs(ex.out)) + (2 * n3 + 4) * ex.pav)
        bo = bo + n3 * SUBNORMAL[dtype]
        bo = bo + _half_ulp(np.abs(ex.out) + bo, dtype)
    bl = F.bounds(ex, D, dtype)[1] if mode == 'dot' else G.bounds(ex, dtype)[1]
    return bo, bl


def check(mode, got_out, got_lse, ex, dtype):
    """got_out: stored elements; got_lse: accumulator numbers -> (ratio of out, ratio of lse)."""
    bo, bl = bounds(mode, ex, dtype)
    g = to_acc(got_out, dtype).astype(np.float64)
    return (_ratio(g, ex.out, bo, 'out', dtype), _ratio(np.asarray(got_lse, np.float64), ex.lse, bl, 'lse', dtype))


def rejects(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


# ---- backward oracle -----------------------------------------------------------------------------------------------
def _scores(mode, ptr, ind, bias, sr, sc, scalar):
    """-> (s, mass, d s / d z, z or None), [E, H] fp64."""
    sr, sc = np.asarray(sr, np.float64), np.asarray(sc, np.float64)
    M, E = sr.shape[0], len(ind)
    if mode == 'gat':
        z, mass = G.preact(ptr, ind, bias, sr, sc)
        return G.leaky(z, scalar), mass, np.where(z > 0, 1.0, scalar), z
    row = _seg_of(ptr, M, E)
    b = _bias_rows(bias, E, sr.shape[1])
    with np.errstate(invalid='ignore', over='ignore'):
        t = LD(scalar) * sr[row].astype(LD) * sc[ind].astype(LD)
        s = (t.sum(-1) + b).astype(np.float64)
        mass = np.abs(t).sum(-1).astype(np.float64) + np.abs(b)
    return s, mass, np.ones_like(s), None


def bw_exact(mode, ptr, ind, bias, sr, sc, v, out, lse, go, scalar, keep, c, dtype):
    """What the backward kernel computes FROM THE GIVEN out and lse -> (pt [E, H], d [E, H], bound of pt, bound of d), d =
    ds (dot) or dz (gat); the bounds are those of the accumulator values, before the store.
        pt = p keep c,   ds = p (keep c dp - delta),   dz = ds (z > 0 ? 1 : slope).
    p carries the plain call's relative error `rel` u; pt two more roundings (c, the product); ds the same, the
    subtraction and the product, and the two dot products' (D + 3) u sum |terms| with the dp side weighted by keep c."""
    v, out, lse, go = (np.asarray(a, np.float64) for a in (v, out, lse, go))
    M, E, D = out.shape[0], len(ind), v.shape[2]
    u = U[dtype]
    ks = D + 3 if mode == 'dot' else G.KSCORE
    row = _seg_of(ptr, M, E)
    s, mass, factor, z = _scores(mode, ptr, ind, bias, sr, sc, scalar)
    kc = np.asarray(keep, np.float64) * c
    with np.errstate(invalid='ignore', over='ignore'):
        dp = (go[row].astype(LD) * v[ind].astype(LD)).sum(-1).astype(np.float64)
        dl = (go[row].astype(LD) * out[row].astype(LD)).sum(-1).astype(np.float64)
        mv, mo = np.abs(go[row] * v[ind]).sum(-1), np.abs(go[row] * out[row]).sum(-1)
        ls = lse[row]
        p = np.exp(s - ls)
        pt = p * kc
        ds = p * (kc * dp - dl)
        d = ds * factor
        dead = ~np.isfinite(ls)
        pt[dead], d[dead], ds[dead] = np.nan, np.nan, np.nan
        masked = np.isneginf(s) & ~dead
        pt[masked], d[masked], ds[masked] = 0.0, 0.0, 0.0
        dist = np.abs(np.where(np.isfinite(s - ls), s - ls, 0.0))
        rel = ks * mass + np.abs(ls) + 2 * dist + 6
        bpt = u * pt * (rel + 2)
        bd = u * (np.abs(d) * (rel + 6) + p * np.abs(factor) * ((D + 3) * (kc * mv + mo) + 2 * kc * np.abs(dp)))
        if z is not None:
            unsure = (z != 0) & (np.abs(z) <= 2 * u * mass)
            bd = bd + np.where(unsure, np.abs(ds) * abs(1.0 - scalar), 0.0)
    return pt, d, bpt, bd


def check_bw(got_pt, got_d, expect, dtype):
    pt, d, bpt, bd = expect
    return tuple(_ratio(to_acc(got, dtype).astype(np.float64), ref, G.stored_bound(ref, b, dtype), what, dtype)
                 for got, ref, b, what in ((got_pt, pt, bpt, 'pt'), (got_d, d, bd, 'd')))


def grads_exact(mode, ptr, ind, bias, sr, sc, v, scalar, go, keep, c, dtype='f64', out=None, lse=None):
    """The four gradients of sum(go * call(...)) as sums of the backward's pt and d, loops over the rows and their entries
    -> (Grads of references, Grads of bounds); bias is [E, H].  out / lse: the forward results the backward is given
    (None: the oracle's own).  dot: grad_sr[r] = scale sum d k, grad_sc[n] = scale sum d q; gat: the sums of dz over the
    rows and the columns.  grad_v[n] = sum pt go.  The bound of a gradient is the bound of the stored factor times the
    other one summed over the segment, the segment sum's own (2 n + 2) u sum |terms|, and half an ulp of the stored
    type.  The dot mode's two sums are stored UNSCALED -- half an ulp at that magnitude -- and then multiplied by the
    scale in place: the bound so far times |scale|, the product's rounding in the accumulator, and half an ulp of the
    scaled value.  (Half an ulp is not scale invariant: at the unscaled magnitude it can be twice the scaled one's.)"""
    sr, sc, v, go = (np.asarray(a, np.float64) for a in (sr, sc, v, go))
    ptr, ind = np.asarray(ptr, np.int64), np.asarray(ind, np.int64)
    if out is None:
        ex = exact_dropout(plain_exact(mode, ptr, ind, bias, sr, sc, v, scalar), ptr, ind, v, keep, c)
        out, lse = ex.out, ex.lse
    pt, d, bpt, bd = bw_exact(mode, ptr, ind, bias, sr, sc, v, out, lse, go, scalar, keep, c, dtype)
    bpt, bd = G.stored_bound(pt, bpt, dtype), G.stored_bound(d, bd, dtype)
    u = U[dtype]
    M, N = sr.shape[0], sc.shape[0]
    g = [np.zeros(a.shape, LD) for a in (sr, sc, v)]
    b = [np.zeros(a.shape, LD) for a in (sr, sc, v)]
    a = [np.zeros(a.shape, LD) for a in (sr, sc, v)]
    dot = mode == 'dot'
    for r in range(M):
        for e in range(int(ptr[r]), int(ptr[r + 1])):
            n = ind[e]
            wr = sc[n] if dot else 1.0   # what d multiplies on the row side, [H, D] or a scalar; the scale comes last
            wc = sr[r] if dot else 1.0
            dr = d[e][:, None] if dot else d[e]
            br = bd[e][:, None] if dot else bd[e]
            g[0][r] += dr * wr
            b[0][r] += br * np.abs(wr)
            a[0][r] += np.abs(dr * wr)
            g[1][n] += dr * wc
            b[1][n] += br * np.abs(wc)
            a[1][n] += np.abs(dr * wc)
            g[2][n] += pt[e][:, None] * go[r]
            b[2][n] += bpt[e][:, None] * np.abs(go[r])
            a[2][n] += np.abs(pt[e][:, None] * go[r])
    nr = np.diff(ptr[:M + 1]).astype(np.float64)
    nc = np.bincount(ind, minlength=N).astype(np.float64)
    shape = lambda cnt, like: cnt.reshape((-1, ) + (1, ) * (like.ndim - 1))  # noqa: E731

    def close(ref, bnd, own, cnt, scaled):
        ref, bnd = ref.astype(np.float64), (bnd + own).astype(np.float64) + cnt * SUBNORMAL[dtype]
        with np.errstate(invalid='ignore'):
            bnd = bnd + _half_ulp(np.abs(ref) + bnd, dtype)
            if scaled:
                ref, bnd = ref * scalar, bnd * abs(scalar) + u * np.abs(ref * scalar) + SUBNORMAL[dtype]
                bnd = bnd + _half_ulp(np.abs(ref) + bnd, dtype)
        return ref, bnd

    gsr, bsr = close(g[0], b[0], (2 * shape(nr, sr) + 2) * u * a[0], shape(nr, sr), dot)
    gsc, bsc = close(g[1], b[1], (2 * shape(nc, sc) + 2) * u * a[1], shape(nc, sc), dot)
    gv, bv = close(g[2], b[2], (2 * shape(nc, v) + 2) * u * a[2], shape(nc, v), False)
    return Grads(gsr, gsc, gv, d), Grads(bsr, bsc, bv, bd)


def check_grads(got, expect, dtype, shared_bias=False):
    """got: Grads of stored elements, None where a gradient was not asked for -> the worst error / bound of each."""
    grads, bnd = expect
    res = []
    for name in Grads._fields:
        gt = getattr(got, name)
        if gt is None:
            continue
        ref, b = getattr(grads, name), getattr(bnd, name)
        if name == 'bias' and shared_bias:
            ref, b = G.bias_shared(G.Grads(None, None, None, grads.bias), G.Grads(None, None, None, bnd.bias), dtype)
        res.append(_ratio(to_acc(gt, dtype).astype(np.float64), ref, b, 'grad_' + name, dtype))
    return tuple(res)


# ---- torch on the CPU ----------------------------------------------------------------------------------------------
def _torch_scores(mode, sr, sc, rows, cols, bias_rows, scalar):
    """[n, H] scores of the entries (rows[i], cols[i]) in the dtype of the operands."""
    import torch
    if mode == 'dot':
        s = (sr[rows] * sc[cols]).sum(-1) * scalar
        return s if bias_rows is None else s + bias_rows
    z = sr[rows] + sc[cols]
    if bias_rows is not None:
        z = z + bias_rows
    return torch.nn.functional.leaky_relu(z, scalar)


def dense_torch(mode, mask, row, col, bias, sr, sc, v, scalar, keep, c):
    """Dense masked torch in the dtype of the operands (tensors; autograd flows): softmax over the row, multiply by the
    scattered mask times c, matmul.  mask [M, N] bool with (row, col) its entries in CSR order; bias None / [E] / [E, H]
    tensor; keep [E, H] -> out [M, H, D]; rows without entries give zeros."""
    import torch
    M, N = mask.shape
    H = v.size(1)
    rr, cc = torch.from_numpy(np.asarray(row, np.int64)), torch.from_numpy(np.asarray(col, np.int64))
    b = None if bias is None else (bias if bias.dim() == 2 else bias[:, None].expand(-1, H))
    s = _torch_scores(mode, sr, sc, rr, cc, b, scalar)                         # [E, H]
    scores = torch.full((M, N, H), -np.inf, dtype=v.dtype).index_put((rr, cc), s)
    P = torch.softmax(scores, 1)
    m3 = torch.from_numpy(np.asarray(mask))[:, :, None].expand_as(P)
    P = torch.where(m3 & ~torch.isnan(P), P, torch.zeros_like(P))
    W = torch.zeros((M, N, H), dtype=v.dtype).index_put((rr, cc), torch.from_numpy(np.asarray(keep, np.float64) * c).to(v.dtype))
    return torch.einsum('mnh,nhd->mhd', P * W, v)


def composition_f32(mode, ptr, ind, bias, sr, sc, v, scalar, keep, c):
    """The chain in float32 torch on the CPU, row by row: scores, torch.softmax, the mask times c, weighted sum -> (out,
    lse)."""
    import torch
    sr, sc, v = (torch.from_numpy(np.asarray(a, np.float32)) for a in (sr, sc, v))
    M, H, D = sr.shape[0], v.shape[1], v.shape[2]
    E = len(ind)
    b = None if bias is None else torch.from_numpy(_bias_rows(bias, E, H).astype(np.float32))
    w = torch.from_numpy((np.asarray(keep, np.float64) * c).astype(np.float32))
    out, lse = torch.zeros(M, H, D), torch.full((M, H), -np.inf)
    col = torch.from_numpy(np.asarray(ind, np.int64))
    for r in range(M):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        if lo == hi:
            continue
        rows = torch.full((hi - lo, ), r, dtype=torch.int64)
        s = _torch_scores(mode, sr, sc, rows, col[lo:hi], None if b is None else b[lo:hi], np.float32(scalar).item())
        out[r] = ((torch.softmax(s, 0) * w[lo:hi])[:, :, None] * v[col[lo:hi]]).sum(0)
        lse[r] = torch.logsumexp(s, 0)
    return out.numpy(), lse.numpy()


# ---- the kernel by pieces, with planted defects ---------------------------------------------------------------------
def _emulated_scores(mode, ptr, ind, bias, sr, sc, scalar, chunk, dtype):
    """s [E, H] in the accumulator type, as the tile kernel forms it."""
    if mode == 'gat':
        return G.emulate_scores(ptr, ind, bias, sr, sc, scalar, chunk, dtype)
    A = ACC[dtype]
    sr, sc = np.asarray(sr).astype(A), np.asarray(sc).astype(A)
    E = len(ind)
    row = _seg_of(ptr, sr.shape[0], E)
    b = _bias_rows(bias, E, sr.shape[1]).astype(A)
    with np.errstate(invalid='ignore', over='ignore'):
        return ((sr[row] * sc[ind]).sum(-1, dtype=A) * A(scalar) + b).astype(A)


def emulate(mode, ptr, ind, bias, sr, sc, v, scalar, chunk, dtype, seed, rate, mutant=None, lpr=2):
    """The call with dropout restated by composition: the scores as the kernel forms them, then F.emulate -- the chunk /
    record / fix-up scheme with the online combine -- on the pattern in which every entry gathers a source row of its
    own, v[col] times keep c in the accumulator type, fed the scores as its bias beside a zero dot product.  So l folds
    every entry and only the accumulator row sees the mask -> (out, lse) in the accumulator type.  `mutant` plants a
    defect of FW_MUTANTS (lpr: the group width of 'batch_aligned_to_window')."""
    assert mutant is None or mutant in FW_MUTANTS
    A = ACC[dtype]
    v = np.asarray(v).astype(A)
    ptr, ind = np.asarray(ptr, np.int64), np.asarray(ind, np.int64)
    E, H = len(ind), v.shape[1]
    s = _emulated_scores(mode, ptr, ind, bias, sr, sc, scalar, chunk, dtype)
    keep = keep_mask(seed, rate, E, H)
    cc = A(1.0 if mutant == 'c_missing' else scale_of(rate))
    if mutant == 'mask_of_next_entry':
        keep = np.concatenate([keep[1:], keep[:1]])
    elif mutant == 'mask_shared_between_heads':
        keep = np.repeat(keep[:, :1], H, 1)
    elif mutant == 'keep_inverted':
        keep = ~keep
    elif mutant == 'batch_aligned_to_window':
        keep = keep_mask_by_window(seed, rate, E, H, lpr)
    if mutant == 'l_masked_too':  # a dropped entry leaves the softmax altogether: renormalised dropout
        s = np.where(keep, s, A(-np.inf)).astype(A)
    vv = (v[ind] * (keep.astype(A) * cc)[:, :, None]).astype(A)
    zq = np.zeros((len(ptr) - 1, ) + v.shape[1:])
    return F.emulate(ptr, np.arange(E, dtype=np.int64), s, zq, np.zeros(vv.shape), vv, 1.0, chunk, dtype)


def emulate_bw(mode, ptr, ind, bias, sr, sc, v, out, lse, go, scalar, dtype, seed, rate, mutant=None):
    """The backward kernel restated in the accumulator type -> (pt, d) as stored elements."""
    assert mutant is None or mutant in BW_MUTANTS
    A = ACC[dtype]
    sr, sc, v, out, go = (np.asarray(a).astype(A) for a in (sr, sc, v, out, go))
    lse = np.asarray(lse).astype(A)
    E, H = len(ind), v.shape[1]
    row = _seg_of(ptr, sr.shape[0], E)
    b = _bias_rows(bias, E, H).astype(A)
    kc = keep_mask(seed, rate, E, H).astype(A) * A(scale_of(rate))
    with np.errstate(invalid='ignore', over='ignore'):
        if mode == 'gat':
            z = (sr[row] + sc[ind]) + b
            s = np.where(z > 0, z, z * A(scalar))
            factor = np.where(z > 0, A(1), A(scalar))
        else:
            s = (sr[row] * sc[ind]).sum(-1, dtype=A) * A(scalar) + b
            factor = np.ones_like(s)
        dp = (go[row] * v[ind]).sum(-1, dtype=A)
        dl = (go[row] * out[row]).sum(-1, dtype=A)
        ls = lse[row]
        p = np.exp(s - ls).astype(A)
        pt = p if mutant == 'grad_v_uses_p' else p * kc
        d = p * ((dp if mutant == 'dp_without_keep_c' else kc * dp) - dl) * factor
        dead = ~np.isfinite(ls)
        pt[dead], d[dead] = np.nan, np.nan
        masked = np.isneginf(s) & ~dead
        pt[masked], d[masked] = 0, 0
    return store(pt, dtype), store(d, dtype)
