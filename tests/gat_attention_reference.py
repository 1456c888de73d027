"""Reference of the fused additive (GAT) attention (csrc/attention.hip in its additive score mode): an fp64 oracle of the
forward (out, lse, p, z) and of everything the backward computes (p, dz, the four gradients) written as loops over the
rows and their entries, the comparators with a derived bound, operand sets with a host census of the pre-activation,
and a numpy restatement of how the kernel forms the scores (chunks, the a_dst reload where the segment changes) and the
gradients, whose switches plant defects.  The online softmax, the records and the fix-up are those of
tests/fused_attention_reference.py: its `emulate` is fed the scores.  numpy only.

    z(i, h) = a_dst[r, h] + a_src[col[i], h] (+ bias[i] or bias[i, h]),   s = z > 0 ? z : negative_slope * z

The bound (derived in docs/design/widening.md, "Additive attention") is that of the fused dot-product call with the
score term replaced.  u is the unit roundoff of the accumulator A, mass_i = |a_dst| + |a_src| + |bias|.  The kernel
forms z with at most two additions in A (the operands convert exactly), |z' - z| <= 2 u mass to first order; the
activation is 1-Lipschitz for |negative_slope| <= 1, also where z' and z differ in sign; the negative side multiplies by
the slope (its conversion to A and the product: two roundings, 2 u |slope| |z| <= 2 u mass).  So |s' - s| <= KSCORE u
mass_i with KSCORE = 4, in place of (D + 3) u mass_i.  Everything else -- the arguments of e, the factors per change of
the maximum, the two sums, the division, the store -- is unchanged."""
from collections import namedtuple

import numpy as np

from tests import fused_attention_reference as F
from tests.attention_reference import LD, SUBNORMAL, U, _half_ulp, _seg_of, csc_of, numbers  # noqa: F401
from tests.fused_attention_reference import _bias_rows, _ratio
from tests.segreduce_reference import ACC, store, to_acc  # noqa: F401

KSCORE = 4  # two additions, the slope's conversion and the product
FLOATS = F.FLOATS
PEAKS = F.PEAKS
SCORE_MUTANTS = ('slope_on_positive_side', 'bias_outside_activation', 'a_src_by_row', 'a_dst_of_previous_row',
                 'head_dropped')
GRAD_MUTANTS = ('dz_without_slope', 'grad_a_src_by_rows', 'derivative_one_at_zero')

Expect = namedtuple('Expect', F.Expect._fields + ('z', ))
Operands = namedtuple('Operands', 'a_dst a_src v bias')
Grads = namedtuple('Grads', 'a_dst a_src v bias')


def leaky(z, slope):
    """torch's leaky_relu: z > 0 ? z : z * slope, also at z == 0 and for NaN; 0 * -inf is NaN."""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(z > 0, z, z * slope)


# ---- oracle --------------------------------------------------------------------------------------------------------
def preact(ptr, ind, bias, a_dst, a_src):
    """-> (z [E, H] fp64, mass [E, H]): a loop over the rows and their entries."""
    a_dst, a_src = np.asarray(a_dst, np.float64), np.asarray(a_src, np.float64)
    M, H = a_dst.shape
    E = len(ind)
    b = _bias_rows(bias, E, H)
    z, mass = np.zeros((E, H)), np.zeros((E, H))
    with np.errstate(invalid='ignore'):
        for r in range(M):
            for i in range(int(ptr[r]), int(ptr[r + 1])):
                z[i] = (a_dst[r].astype(LD) + a_src[ind[i]].astype(LD) + b[i].astype(LD)).astype(np.float64)
                mass[i] = np.abs(a_dst[r]) + np.abs(a_src[ind[i]]) + np.abs(b[i])
    return z, mass


def exact(ptr, ind, bias, a_dst, a_src, v, slope):
    """a_dst [M, H], a_src [N, H], v [N, H, D] numbers, bias None / [E] / [E, H] -> Expect.  Per row and head: m = max s,
    p = exp(s - m) / sum; a NaN or +inf score or a row of -inf only makes out NaN (lse NaN, -inf for the row of -inf)."""
    a_dst, a_src, v = (np.asarray(a, np.float64) for a in (a_dst, a_src, v))
    ptr, ind = np.asarray(ptr, np.int64), np.asarray(ind, np.int64)
    M, H = a_dst.shape
    D = v.shape[2]
    E = len(ind)
    z_all, mass_all = preact(ptr, ind, bias, a_dst, a_src)
    s_all = leaky(z_all, slope)
    out, pav, a1, a2 = (np.zeros((M, H, D)) for _ in range(4))
    lse = np.full((M, H), -np.inf)
    b1, b2, m_, logl = (np.zeros((M, H)) for _ in range(4))
    p_all = np.zeros((E, H))
    n = np.diff(ptr[:M + 1])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for r in range(M):
            lo, hi = int(ptr[r]), int(ptr[r + 1])
            if lo == hi:
                continue
            vv = v[ind[lo:hi]]                                        # [n, H, D]
            s, mass = s_all[lo:hi], mass_all[lo:hi]
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
            p_all[lo:hi] = p
    return Expect(out, lse, n, pav, a1, a2, b1, b2, m_, logl, p_all, s_all, mass_all, z_all)


def bounds(ex, dtype):
    """fused_attention_reference.bounds with (D + 3) u mass replaced by KSCORE u mass -> (bound of out, bound of lse)."""
    u = U[dtype]
    n = ex.n.astype(np.float64)
    n3, n2 = n[:, None, None], n[:, None]
    with np.errstate(invalid='ignore'):
        bo = u * (KSCORE * ex.a1 + 2 * ex.a2 + (5 * n3 + 5) * (ex.pav + np.abs(ex.out)) + (2 * n3 + 2) * ex.pav)
        bo = bo + n3 * SUBNORMAL[dtype]
        bo = bo + _half_ulp(np.abs(ex.out) + bo, dtype)
        bl = u * (KSCORE * ex.b1 + 2 * ex.b2 + (5 * n2 + 5) + (n2 + 2) + 3 * (np.abs(ex.m) + np.abs(ex.logl)) +
                  np.abs(ex.lse))
    return bo, bl


def check(got_out, got_lse, ex, dtype):
    """got_out: stored elements [M, H, D]; got_lse: accumulator numbers [M, H].  Non-finite exactly where and as the
    oracle has it, rows without entries exactly zero / -inf, elsewhere inside the bound -> (ratio of out, ratio of lse)."""
    bo, bl = bounds(ex, dtype)
    g = to_acc(got_out, dtype).astype(np.float64)
    return (_ratio(g, ex.out, bo, 'out', dtype), _ratio(np.asarray(got_lse, np.float64), ex.lse, bl, 'lse', dtype))


def rejects(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def bw_exact(ptr, ind, bias, a_dst, a_src, v, out, lse, go, slope, dtype):
    """What tsamd_gat_attention_heads_bw computes FROM THE GIVEN out and lse -> (p [E, H], dz [E, H], bound of p, bound
    of dz): the bounds are those of the accumulator values, before the store.  Of p as in the dot-product call with the
    score term replaced; ds = p * (dp - delta) two more roundings and the two dot products' (D + 3) u sum|terms|; dz
    one more product and the slope's conversion.  Where z is not zero but within its own error 2 u mass of zero the
    kernel may take the other branch of the derivative: |ds| |1 - slope| more."""
    a_dst, a_src, v, out, lse, go = (np.asarray(a, np.float64) for a in (a_dst, a_src, v, out, lse, go))
    M, H = a_dst.shape
    D = v.shape[2]
    E = len(ind)
    u = U[dtype]
    row = _seg_of(ptr, M, E)
    z, mass = preact(ptr, ind, bias, a_dst, a_src)
    s = leaky(z, slope)
    with np.errstate(invalid='ignore', over='ignore'):
        dp = (go[row].astype(LD) * v[ind].astype(LD)).sum(-1).astype(np.float64)
        dl = (go[row].astype(LD) * out[row].astype(LD)).sum(-1).astype(np.float64)
        mdp = (np.abs(go[row] * v[ind])).sum(-1) + (np.abs(go[row] * out[row])).sum(-1)
        ls = lse[row]
        p = np.exp(s - ls)
        ds = p * (dp - dl)
        factor = np.where(z > 0, 1.0, slope)
        dz = ds * factor
        dead = ~np.isfinite(ls)
        p[dead], dz[dead], ds[dead] = np.nan, np.nan, np.nan
        masked = np.isneginf(s) & ~dead
        p[masked], dz[masked], ds[masked] = 0.0, 0.0, 0.0
        dist = np.abs(np.where(np.isfinite(s - ls), s - ls, 0.0))
        rel = KSCORE * mass + np.abs(ls) + 2 * dist + 6      # of p, in units of u
        bp = u * p * rel
        bd = u * (np.abs(dz) * (rel + 4) + p * (D + 3) * mdp * np.abs(factor))
        unsure = (z != 0) & (np.abs(z) <= 2 * u * mass)
        bd = bd + np.where(unsure, np.abs(ds) * abs(1.0 - slope), 0.0)
    return p, dz, bp, bd


def stored_bound(ref, b, dtype):
    """The bound of an accumulator value -> of the stored element: a subnormal step and half an ulp of the type."""
    with np.errstate(invalid='ignore'):
        bound = b + SUBNORMAL[dtype] * (ref != 0)
        return np.where(np.isfinite(bound), bound + _half_ulp(np.abs(ref) + bound, dtype) * (ref != 0), bound)


def check_bw(got_p, got_dz, expect, dtype):
    p, dz, bp, bd = expect
    return tuple(_ratio(to_acc(got, dtype).astype(np.float64), ref, stored_bound(ref, b, dtype), what, dtype)
                 for got, ref, b, what in ((got_p, p, bp, 'p'), (got_dz, dz, bd, 'dz')))


def grads_exact(ptr, ind, bias, a_dst, a_src, v, slope, go, dtype='f64', out=None, lse=None):
    """The four gradients of sum(go * gat_attention(a_dst, a_src, v)) as sums of the backward's p and dz, loops over the
    rows and their entries -> (Grads of references, Grads of bounds); bias is [E, H] (sum over the heads for a [E] bias:
    bias_shared).  out / lse: the forward results the backward is given (None: the oracle's own).  The bound of a
    gradient is the bound of the stored dz (p times |go| for v) summed over the segment, plus the segment sum's own
    n u sum|terms| (2 n + 2 for v: a product and a sum), plus half an ulp of the stored type."""
    a_dst, a_src, v, go = (np.asarray(a, np.float64) for a in (a_dst, a_src, v, go))
    if out is None:
        ex = exact(ptr, ind, bias, a_dst, a_src, v, slope)
        out, lse = ex.out, ex.lse
    p, dz, bp, bd = bw_exact(ptr, ind, bias, a_dst, a_src, v, out, lse, go, slope, dtype)
    bp, bd = stored_bound(p, bp, dtype), stored_bound(dz, bd, dtype)
    u = U[dtype]
    gd, bgd, ad = (np.zeros(a_dst.shape, LD) for _ in range(3))
    gs, bgs, as_ = (np.zeros(a_src.shape, LD) for _ in range(3))
    gv, bgv, av = (np.zeros(v.shape, LD) for _ in range(3))
    M = a_dst.shape[0]
    for r in range(M):
        for e in range(int(ptr[r]), int(ptr[r + 1])):
            c = ind[e]
            gd[r] += dz[e]
            bgd[r] += bd[e]
            ad[r] += np.abs(dz[e])
            gs[c] += dz[e]
            bgs[c] += bd[e]
            as_[c] += np.abs(dz[e])
            gv[c] += p[e][:, None] * go[r]
            bgv[c] += bp[e][:, None] * np.abs(go[r])
            av[c] += np.abs(p[e][:, None] * go[r])
    nr = np.diff(np.asarray(ptr, np.int64)[:M + 1]).astype(np.float64)
    nc = np.bincount(ind, minlength=a_src.shape[0]).astype(np.float64)
    f = np.float64

    def close(ref, b, own):
        ref, b = ref.astype(f), (b + own).astype(f)
        with np.errstate(invalid='ignore'):
            return ref, b + _half_ulp(np.abs(ref) + b, dtype)

    gd, bgd = close(gd, bgd, nr[:, None] * u * ad)
    gs, bgs = close(gs, bgs, nc[:, None] * u * as_)
    gv, bgv = close(gv, bgv, (2 * nc[:, None, None] + 2) * u * av + nc[:, None, None] * SUBNORMAL[dtype])
    return Grads(gd, gs, gv, dz), Grads(bgd, bgs, bgv, bd)


def bias_shared(grads, bounds_, dtype):
    """(reference, bound) of the gradient of a [E] bias: dz summed over the H heads in the accumulator, stored once."""
    H = grads.bias.shape[1]
    ref = grads.bias.sum(1)
    b = bounds_.bias.sum(1) + H * U[dtype] * np.abs(grads.bias).sum(1)
    with np.errstate(invalid='ignore'):
        return ref, b + _half_ulp(np.abs(ref) + b, dtype)


def check_grads(got, expect, dtype, shared_bias=False):
    """got: stored elements, None where a gradient was not asked for -> the worst error / bound of each."""
    grads, bnd = expect
    out = []
    for name in Grads._fields:
        g = getattr(got, name)
        if g is None:
            continue
        ref, b = getattr(grads, name), getattr(bnd, name)
        if name == 'bias' and shared_bias:
            ref, b = bias_shared(grads, bnd, dtype)
        out.append(_ratio(to_acc(g, dtype).astype(np.float64), ref, b, 'grad_' + name, dtype))
    return tuple(out)


# ---- operands and their census -------------------------------------------------------------------------------------
def census(ptr, ind, ops, dtype):
    """What the pre-activation of an operand set meets -> {'neg', 'pos': fractions of the (entry, head) pairs, 'zero':
    pairs with z == 0 exactly, 'min_abs': the smallest |z|}."""
    z, _ = preact(ptr, ind, numbers(ops.bias, dtype), numbers(ops.a_dst, dtype), numbers(ops.a_src, dtype))
    return {'neg': float((z < 0).mean()), 'pos': float((z > 0).mean()), 'zero': int((z == 0).sum()),
            'min_abs': float(np.abs(z).min())}


def assert_census(ptr, ind, ops, dtype):
    c = census(ptr, ind, ops, dtype)
    assert c['neg'] >= 0.25 and c['pos'] >= 0.25 and c['zero'] >= 1, c
    return c


def operands(case, dtype, H, D, seed=0, form=0, spread=1.0, bias=None, census_min=64):
    """(a_dst [nseg, H], a_src [nsrc, H], v [nsrc, H, D], bias: form 0 none, 1 [E], 2 [E, H], or the one given) as stored
    elements, with a_dst[r] = -a_src[c] (and a zero bias) planted on the stored entry in the middle of the longest row, so
    that z == 0 exactly there; the census is asserted (layouts of census_min entries and more: a few entries have no
    quarters).  spread scales the node terms: with 40 the scores pass +-80."""
    rng = np.random.default_rng(seed)
    a_dst = rng.standard_normal((case.nseg, H)) * spread
    a_src = rng.standard_normal((case.nsrc, H)) * spread
    v = store(rng.standard_normal((case.nsrc, H, D)), dtype)
    if bias is None and form:
        bias = rng.standard_normal(case.E if form == 1 else (case.E, H))
    a_src = store(a_src, dtype)
    r = int(np.argmax(np.diff(case.ptr)))
    e = (int(case.ptr[r]) + int(case.ptr[r + 1])) // 2
    a_dst[r] = -numbers(a_src, dtype)[case.ind[e]]
    a_dst = store(a_dst, dtype)
    if bias is not None:
        bias = np.array(bias, np.float64)
        bias[e] = 0.0
        bias = store(bias, dtype)
    ops = Operands(a_dst, a_src, v, bias)
    if case.E >= census_min:
        assert_census(case.ptr, case.ind, ops, dtype)
    return ops


def gradcheck_operands(ptr, ind, M, N, H, D, seed=0):
    """fp64 operands (numbers) of a tiny graph for torch.autograd.gradcheck: no entry within 1e-2 of the kink -- the
    first seed from `seed` on that has none -> (a_dst, a_src, v, bias [E], bias [E, H])."""
    for s in range(seed, seed + 1000):
        rng = np.random.default_rng(s)
        a_dst, a_src, v = rng.standard_normal((M, H)), rng.standard_normal((N, H)), rng.standard_normal((N, H, D))
        b1, b2 = rng.standard_normal(len(ind)), rng.standard_normal((len(ind), H))
        if all(float(np.abs(preact(ptr, ind, b, a_dst, a_src)[0]).min()) >= 1e-2 for b in (None, b1, b2)):
            return a_dst, a_src, v, b1, b2
    raise AssertionError('no seed keeps every |z| above 1e-2')


def layouts(dtype, H, D):
    """fused_attention_reference.layouts: (route, [hub, sparse_rows, one_source]) with their census asserted; the additive
    call runs on the lane map of (dtype, H, D) and the route of v and out alone."""
    return F.layouts(dtype, H, D)


Set = namedtuple('Set', 'kind dtype H D layout seed form spread peak')


def gpu_sets(kind=None, dtype=None):
    """Every operand set tests/test_gat_attention_gpu.py runs on a census layout, by the test that uses it (`kind`):
    the CPU suite builds each of them and asserts its census."""
    sets = []
    for dt in FLOATS:
        n = 0
        for H in (1, 2, 3, 8):
            for D in (1, 3, 4, 8, 16, 24, 64):
                sets.append(Set('shape', dt, H, D, 0, 60 + n, n % 3, 1.0, None))
                n += 1
        sets += [Set('backward', dt, 3, 8, 0, 130, 2, 1.0, None), Set('backward', dt, 2, 5, 0, 131, 1, 1.0, None),
                 Set('backward', dt, 3, 8, 2, 132, 0, 1.0, None)]
        sets += [Set('public', dt, 3, 8, 0, 140, form, 1.0, None) for form in (2, 1, 0)]
    sets += [Set('wide', 'f32', 1, 264, 0, 70, 2, 1.0, None), Set('wide', 'bf16', 1, 520, 0, 70, 2, 1.0, None)]
    for dt in ('f32', 'bf16'):
        sets += [Set('layout', dt, 3, 8, li, 80 + li, li % 3, 1.0, None) for li in range(3)]
        sets += [Set('peak', dt, 3, 8, 0, 90, 1, 1.0, where) for where in PEAKS]
        sets.append(Set('large', dt, 3, 8, 0, 91, 0, 40.0, None))
    sets += [Set('nan', 'f32', 3, 8, 0, 110, 0, 1.0, None), Set('minus_inf', 'f32', 3, 8, 0, 120, 2, 1.0, None),
             Set('flat', 'f32', 1, 6, 0, 150, 0, 1.0, None), Set('caches', 'f32', 2, 5, 0, 151, 1, 1.0, None),
             Set('script', 'f32', 3, 8, 0, 152, 0, 1.0, None)]
    return [s for s in sets if (kind is None or s.kind == kind) and (dtype is None or s.dtype == dtype)]


def build(s):
    """A Set -> (route, layout, operands): the census of the layout and of the operands asserted on the host."""
    r, cases = layouts(s.dtype, s.H, s.D)
    assert r.chunk <= 512
    case = cases[s.layout]
    bias = F.peak_bias(case, r.chunk, s.peak) if s.peak else None
    return r, case, operands(case, s.dtype, s.H, s.D, seed=s.seed, form=s.form, spread=s.spread, bias=bias, census_min=1)


# ---- torch on the CPU ----------------------------------------------------------------------------------------------
def composition_f32(ptr, ind, bias, a_dst, a_src, v, slope):
    """The chain in float32 torch on the CPU, row by row: leaky_relu(a_dst[row] + a_src[col] + b), torch.softmax, weighted
    sum -> (out, lse)."""
    import torch
    a_dst, a_src, v = (torch.from_numpy(np.asarray(a, np.float32)) for a in (a_dst, a_src, v))
    M, H = a_dst.shape
    D = v.shape[2]
    b = None if bias is None else torch.from_numpy(_bias_rows(bias, len(ind), H).astype(np.float32))
    out, lse = torch.zeros(M, H, D), torch.full((M, H), -np.inf)
    col = torch.from_numpy(np.asarray(ind, np.int64))
    for r in range(M):
        lo, hi = int(ptr[r]), int(ptr[r + 1])
        if lo == hi:
            continue
        z = a_dst[r][None] + a_src[col[lo:hi]]
        if b is not None:
            z = z + b[lo:hi]
        s = torch.nn.functional.leaky_relu(z, slope)
        out[r] = (torch.softmax(s, 0)[:, :, None] * v[col[lo:hi]]).sum(0)
        lse[r] = torch.logsumexp(s, 0)
    return out.numpy(), lse.numpy()


# ---- the kernel by pieces, with planted defects ---------------------------------------------------------------------
def emulate_scores(ptr, ind, bias, a_dst, a_src, slope, chunk, dtype, mutant=None):
    """How the tile kernel forms the scores, in the accumulator type of `dtype`: every chunk walks its entries in order,
    holds a_dst of the row it is in and reloads it where the segment changes, gathers a_src by column, adds the bias
    inside the activation -> s [E, H]."""
    assert mutant is None or mutant in SCORE_MUTANTS
    A = ACC[dtype]
    a_dst, a_src = np.asarray(a_dst).astype(A), np.asarray(a_src).astype(A)
    M, H = a_dst.shape
    E = len(ind)
    b = _bias_rows(bias, E, H).astype(A)
    seg = _seg_of(ptr, M, E)
    sl = A(slope)
    s = np.zeros((E, H), A)
    with np.errstate(invalid='ignore', over='ignore'):
        for c0 in range(0, E, chunk):
            held, dst = -1, None
            for i in range(c0, min(c0 + chunk, E)):
                r = seg[i]
                if r != held and not (mutant == 'a_dst_of_previous_row' and held >= 0):
                    held, dst = r, a_dst[r]
                src = a_src[min(r, a_src.shape[0] - 1)] if mutant == 'a_src_by_row' else a_src[ind[i]]
                d = dst
                if mutant == 'head_dropped':
                    d, src = np.full(H, d[0], A), np.full(H, src[0], A)
                if mutant == 'bias_outside_activation':
                    z = d + src
                    s[i] = np.where(z > 0, z, z * sl) + b[i]
                    continue
                z = (d + src) + b[i]
                s[i] = np.where(z < 0, z, z * sl) if mutant == 'slope_on_positive_side' else np.where(z > 0, z, z * sl)
    return s


def emulate(ptr, ind, bias, a_dst, a_src, v, slope, chunk, dtype, mutant=None):
    """The additive call restated: emulate_scores, then the chunk / record / fix-up scheme of the dot-product call
    (fused_attention_reference.emulate) fed these scores as its bias beside a zero dot product -> (out, lse)."""
    s = emulate_scores(ptr, ind, bias, a_dst, a_src, slope, chunk, dtype, mutant)
    v = np.asarray(v)
    zq = np.zeros((np.asarray(a_dst).shape[0], ) + v.shape[1:])
    return F.emulate(ptr, ind, s, zq, np.zeros(v.shape), v, 1.0, chunk, dtype)


def emulate_grads(ptr, ind, bias, a_dst, a_src, v, out, lse, go, slope, dtype, mutant=None):
    """The backward restated in the accumulator type: p and dz per entry as the kernel has them, stored, then summed
    over the rows and the columns -> (p, dz as stored elements, Grads as stored elements)."""
    assert mutant is None or mutant in GRAD_MUTANTS
    A = ACC[dtype]
    a_dst, a_src, v, out, go = (np.asarray(a).astype(A) for a in (a_dst, a_src, v, out, go))
    lse = np.asarray(lse).astype(A)
    M, H = a_dst.shape
    N = a_src.shape[0]
    E = len(ind)
    b = _bias_rows(bias, E, H).astype(A)
    row = _seg_of(ptr, M, E)
    sl = A(slope)
    with np.errstate(invalid='ignore', over='ignore'):
        z = (a_dst[row] + a_src[ind]) + b
        s = np.where(z > 0, z, z * sl)
        dp = (go[row] * v[ind]).sum(-1, dtype=A)
        dl = (go[row] * out[row]).sum(-1, dtype=A)
        ls = lse[row]
        p = np.exp(s - ls).astype(A)
        ds = p * (dp - dl)
        kink = z >= 0 if mutant == 'derivative_one_at_zero' else z > 0
        dz = ds if mutant == 'dz_without_slope' else ds * np.where(kink, A(1), sl)
        dead = ~np.isfinite(ls)
        p[dead], dz[dead] = np.nan, np.nan
        masked = np.isneginf(s) & ~dead
        p[masked], dz[masked] = 0, 0
    p, dz = store(p, dtype), store(dz, dtype)
    pa, da = to_acc(p, dtype), to_acc(dz, dtype)
    gd, gs, gv = np.zeros((M, H), A), np.zeros((N, H), A), np.zeros(v.shape, A)
    for e in range(E):
        gd[row[e]] += da[e]
        gs[min(row[e], N - 1) if mutant == 'grad_a_src_by_rows' else ind[e]] += da[e]
        gv[ind[e]] += pa[e][:, None] * go[row[e]]
    return p, dz, Grads(store(gd, dtype), store(gs, dtype), store(gv, dtype), dz)
