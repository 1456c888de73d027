"""Dropout on the probabilities of the fused attention calls (csrc/attention.hip, DROP instantiations) against
tests/attention_dropout_reference.py, both score modes: the forward through the C entry points on the shapes that take
each branch of the mask (per-entry and per-batch Philox, column blocks, generic route, feature blocks), lse and the NaN
positions against the plain call, the mask word for word through the forward and through the backward, the backward's
pt and ds / dz, status codes, and the public calls against dense fp64 torch with the oracle's mask."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_draws as npd
from pytorch_sparse_amd import _native as nat
from tests import attention_dropout_reference as R
from tests import fused_attention_reference as F
from tests import gat_attention_reference as G
from tests.util import bits_equal, fromnp, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
ACC_T = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float32, 'bf16': torch.float32}
GUARD = 64  # elements before and after an output that no call may touch
FW = {'dot': ('tsamd_attention_heads', 'tsamd_attention_heads_dropout'),
      'gat': ('tsamd_gat_attention_heads', 'tsamd_gat_attention_heads_dropout')}
BW = {'dot': ('tsamd_attention_heads_bw', 'tsamd_attention_heads_dropout_bw'),
      'gat': ('tsamd_gat_attention_heads_bw', 'tsamd_gat_attention_heads_dropout_bw')}
SCALAR = {'dot': 0.37, 'gat': 0.2}


@pytest.fixture(scope='module')
def ts(dev):
    import pytorch_sparse_amd
    return pytorch_sparse_amd


def _place(a, tdt, dev, off):
    """A stored numpy array on the device, its first byte at `off` modulo 16."""
    t = fromnp(np.ascontiguousarray(a), tdt)
    raw = torch.zeros(t.numel() * t.element_size() + 32, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    view = raw[off:off + t.numel() * t.element_size()].view(tdt).view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == off
    return view


def _guarded(numel, tdt, dev, off):
    raw = torch.full(((numel + 2 * GUARD) * tdt.itemsize + 32, ), 85, dtype=torch.uint8, device=dev)
    start = off + GUARD * tdt.itemsize
    return raw, start, ctypes.c_void_p(raw.data_ptr() + start)


def _read(raw, start, shape, tdt):
    n = int(np.prod(shape)) * tdt.itemsize
    assert bool((raw[:start] == 85).all()) and bool((raw[start + n:] == 85).all()), 'a byte outside the output was written'
    return raw[start:start + n].clone().view(tdt).view(shape)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(a, b):
    return F.same_bits(np.asarray(a), np.asarray(b))


def call_fw(dev, mode, dtype, case, bias, sr, sc, v, scalar, drop=None, off=0, fill_ws=85):
    """The forward through ctypes into guarded, pre-filled out and lse over a sentinel-filled workspace: the plain entry
    (drop None) or the dropout entry (drop = (rate, seed)) -> (out [M, H, D] stored elements, lse [M, H])."""
    tdt, adt = TORCH[dtype], ACC_T[dtype]
    M, (N, H, D) = sr.shape[0], v.shape
    dsr, dsc = (_place(a, tdt, dev, off if mode == 'dot' else 2 * F.ITEM[dtype] % 16) for a in (sr, sc))
    dv = _place(v, tdt, dev, off)
    db = None if bias is None else _place(bias, tdt, dev, 0)
    dptr, dind = _dev(case.ptr, dev), _dev(case.ind, dev)
    L = nat.lib()
    nbytes = L.tsamd_attention_heads_workspace_bytes(F.CODE[dtype], H, D, case.E)
    assert nbytes == F.workspace_bytes(dtype, H, D, case.E), 'dropout needs no workspace of its own'
    ws = nat.workspace(nbytes, dev)
    ws.fill_(fill_ws)
    raw, start, out = _guarded(M * H * D, tdt, dev, off)
    lraw, lstart, lse = _guarded(M * H, adt, dev, 0)
    name = FW[mode][0 if drop is None else 1]
    extra = () if drop is None else (float(drop[0]), int(drop[1]))
    with torch.cuda.device(dev):
        st = getattr(L, name)(F.CODE[dtype], nat._ptr(dptr), nat._ptr(dind), nat._ptr(db),
                              1 if bias is None or bias.ndim == 1 else H, nat._ptr(dsr), nat._ptr(dsc), nat._ptr(dv),
                              float(scalar), *extra, out, lse, M, N, H, D, case.E, nat._ptr(ws), ctypes.c_size_t(nbytes),
                              nat.stream_ptr(dev))
    nat.check(st, name)
    return tonp(_read(raw, start, (M, H, D), tdt)), tonp(_read(lraw, lstart, (M, H), adt))


def call_bw(dev, mode, dtype, case, bias, sr, sc, v, out, lse, go, scalar, drop, with_row, off=0):
    tdt, adt = TORCH[dtype], ACC_T[dtype]
    M, (N, H, D) = sr.shape[0], v.shape
    dsr, dsc = (_place(a, tdt, dev, off if mode == 'dot' else 0) for a in (sr, sc))
    dv, do, dg = (_place(a, tdt, dev, off) for a in (v, out, go))
    db = None if bias is None else _place(bias, tdt, dev, 0)
    dl = _place(lse, adt, dev, 0)
    row = F._seg_of(case.ptr, M, case.E) if with_row else None
    dptr, dind, drow = (_dev(a, dev) for a in (case.ptr, case.ind, row))
    praw, pstart, p = _guarded(case.E * H, tdt, dev, 0)
    sraw, sstart, ds = _guarded(case.E * H, tdt, dev, 0)
    name = BW[mode][0 if drop is None else 1]
    extra = () if drop is None else (float(drop[0]), int(drop[1]))
    with torch.cuda.device(dev):
        st = getattr(nat.lib(), name)(F.CODE[dtype], nat._ptr(drow), nat._ptr(dptr), nat._ptr(dind), nat._ptr(db),
                                      1 if bias is None or bias.ndim == 1 else H, nat._ptr(dsr), nat._ptr(dsc),
                                      nat._ptr(dv), nat._ptr(do), nat._ptr(dl), nat._ptr(dg), float(scalar), *extra, p, ds,
                                      M, N, H, D, case.E, nat.stream_ptr(dev))
    nat.check(st, name)
    return tonp(_read(praw, pstart, (case.E, H), tdt)), tonp(_read(sraw, sstart, (case.E, H), tdt))


def _operands(mode, case, dtype, H, D, seed, form, spread=1.0):
    """(sr, sc, v, bias) as stored elements; form 0 none, 1 [E], 2 [E, H]."""
    if mode == 'dot':
        q, k, v = F.operands(case, dtype, H, D, seed=seed, spread=spread)
        rng = np.random.default_rng(seed + 1)
        bias = None if form == 0 else F.store(rng.standard_normal(case.E if form == 1 else (case.E, H)), dtype)
        return q, k, v, bias
    ops = G.operands(case, dtype, H, D, seed=seed, form=form, spread=spread, census_min=1 << 30)
    return ops.a_dst, ops.a_src, ops.v, ops.bias


def _numbers(dtype, *arrays):
    return [F.numbers(a, dtype) for a in arrays]


def _oracle(mode, case, dtype, bias, sr, sc, v, scalar, drop, plain=None):
    nsr, nsc, nv, nb = _numbers(dtype, sr, sc, v, bias)
    if plain is None:
        plain = R.plain_exact(mode, case.ptr, case.ind, nb, nsr, nsc, nv, scalar)
    keep = R.keep_mask(drop[1], drop[0], case.E, v.shape[1])
    return plain, R.exact_dropout(plain, case.ptr, case.ind, nv, keep, R.scale_of(drop[0]))


# ---- 1: C-ABI forward against the oracle ------------------------------------------------------------------------------
SHAPES = (  # (H, D), dtypes (None: all four), off, what the f32 / bf16 route must be: (lanes per group, blocks, fblocks, generic)
    ((1, 4), ('f32', ), 0, (1, 1, 1, 0)),       # a group of one lane: Philox per entry
    ((1, 8), ('f32', ), 0, (2, 1, 1, 0)),       # a group of two
    ((2, 8), ('f32', ), 0, (4, 1, 1, 0)),       # a group of four: the batch shares one call from here on
    ((8, 16), None, 0, None),
    ((5, 64), ('f32', ), 0, (64, 2, 1, 0)),     # two column blocks
    ((3, 5), None, 0, None),                    # generic route
    ((4, 64), ('bf16', ), 8, (32, 1, 1, 1)),    # generic by an operand off the 16-byte boundary
    ((1, 300), ('f32', ), 0, (64, 2, 2, 0)),    # WIDE: two feature blocks form the same mask
)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('dtype', F.FLOATS)
def test_cabi_forward_against_the_oracle(dev, mode, dtype):
    """Every shape of the table on the three census layouts, rates 0.1 and 0.6, no bias and [nnz, H] (with one masked entry
    and a row of -inf only: a NaN row): out inside the bound, lse the plain call's bits, NaN where the plain call's is."""
    worst, n = (0.0, 0.0), 0
    for (H, D), dtypes, off, want in SHAPES:
        if dtypes is not None and dtype not in dtypes:
            continue
        r = F.route(dtype, H, D, off == 0)
        if want is not None:
            assert (r.lanes_per_head * r.heads_per_pass, r.blocks, r.fblocks, r.generic) == want, r
        if (H, D) == (3, 5):
            assert r.generic == 1
        _, cases = F.layouts(dtype, H, D)
        for li, case in enumerate(cases):
            combos = ((0.1, 0), (0.6, 2), (0.6, 0), (0.1, 2)) if li == 0 else (((0.6, 2), ) if li == 1 else ((0.1, 0), ))
            plain_of = {}
            for rate, form in combos:
                n += 1
                sr, sc, v, bias = _operands(mode, case, dtype, H, D, 300 + 7 * li + form, form)
                if form == 2 and li == 0:
                    lens = np.diff(case.ptr)
                    hub = int(np.argmax(lens))
                    nb = F.numbers(bias, dtype)
                    nb[case.ptr[hub] + 1] = -np.inf
                    dead = int(np.nonzero((lens >= 2) & (np.arange(lens.size) != hub))[0][0])
                    nb[case.ptr[dead]:case.ptr[dead + 1]] = -np.inf
                    bias = F.store(nb, dtype)
                drop = (rate, 1000 + n)
                plain, ex = _oracle(mode, case, dtype, bias, sr, sc, v, SCALAR[mode], drop, plain_of.get(form))
                plain_of[form] = plain
                out, lse = call_fw(dev, mode, dtype, case, bias, sr, sc, v, SCALAR[mode], drop, off=off, fill_ws=85)
                out2, lse2 = call_fw(dev, mode, dtype, case, bias, sr, sc, v, SCALAR[mode], drop, off=off, fill_ws=0)
                assert _same(out, out2) and _same(lse, lse2), 'two calls differ'
                pout, plse = call_fw(dev, mode, dtype, case, bias, sr, sc, v, SCALAR[mode], None, off=off)
                assert _same(lse, plse), 'lse is the plain call\'s, bit for bit'
                nan_p = np.isnan(F.numbers(pout, dtype))
                assert np.array_equal(np.isnan(F.numbers(out, dtype)), nan_p), 'NaN exactly where the plain call is'
                assert nan_p.any() == (form == 2 and li == 0)
                assert not _same(out, pout)
                try:
                    w = R.check(mode, out, lse, ex, dtype)
                except AssertionError as exc:
                    raise AssertionError('%s: %s' % ((H, D, case.name, rate, form), exc)) from None
                worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    assert n >= 12
    print('%s %s dropout forward: worst err / bound out %.3g lse %.3g over %d calls' % ((mode, dtype) + worst + (n, )))


# ---- 2: rate 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.MODES)
def test_rate_zero_through_the_new_entries_gives_the_plain_bits(dev, mode):
    for dtype, (H, D) in (('f32', (3, 8)), ('bf16', (2, 5)), ('f64', (1, 4))):
        _, cases = F.layouts(dtype, H, D)
        case = cases[0]
        sr, sc, v, bias = _operands(mode, case, dtype, H, D, 400, 2)
        a = call_fw(dev, mode, dtype, case, bias, sr, sc, v, SCALAR[mode], None)
        b = call_fw(dev, mode, dtype, case, bias, sr, sc, v, SCALAR[mode], (0.0, 12345))
        assert _same(a[0], b[0]) and _same(a[1], b[1])
        go = F.store(np.random.default_rng(401).standard_normal(a[0].shape), dtype)
        pa = call_bw(dev, mode, dtype, case, bias, sr, sc, v, a[0], a[1], go, SCALAR[mode], None, True)
        pb = call_bw(dev, mode, dtype, case, bias, sr, sc, v, a[0], a[1], go, SCALAR[mode], (0.0, 12345), True)
        assert _same(pa[0], pb[0]) and _same(pa[1], pb[1])


# ---- 3: the mask word for word through the forward -------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.MODES)
def test_mask_word_for_word_through_the_forward(dev, mode):
    """One entry per row: the probability is 1, so out[r, h] = keep * c * v[col, h] -- all zero iff the oracle drops (r, h)."""
    nrows = 2500
    rng = np.random.default_rng(500)
    case = F.Case('ones', np.arange(nrows + 1, dtype=np.int64), rng.integers(0, 41, nrows).astype(np.int64), nrows, nrows, 41)
    for dtype, H, D in (('f32', 1, 4), ('f32', 1, 8), ('f32', 2, 8), ('f32', 3, 5), ('f16', 8, 16), ('f32', 1, 300)):
        sr, sc, v, _ = _operands(mode, case, dtype, H, D, 501, 0)
        nv = F.numbers(v, dtype)
        v = F.store(np.where(np.abs(nv) < 0.125, 0.5, nv), dtype)  # no zero, nothing that could round to one
        for rate, seed in ((0.6, 2 ** 63 - 1), (0.1, 77)):
            out, lse = call_fw(dev, mode, dtype, case, None, sr, sc, v, SCALAR[mode], (rate, seed))
            keep = R.keep_mask(seed, rate, nrows, H)
            no = F.numbers(out, dtype)
            assert np.array_equal((no != 0).any(2), keep), (dtype, H, D, rate)
            assert np.array_equal((no != 0).all(2), keep), 'a head is kept or dropped whole'
            c = F.ACC[dtype](R.scale_of(rate))
            want = F.store(F.to_acc(v, dtype)[case.ind] * c, dtype)
            assert _same(out[keep], want[keep]), 'p = 1: the value row times c, rounded once'


# ---- 4: the mask through the backward --------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('dtype', F.FLOATS)
@pytest.mark.parametrize('H', [1, 20])
def test_mask_word_for_word_through_the_backward(dev, mode, dtype, H):
    """p_out != 0 is the oracle's mask at every (entry, head); H = 20 takes two backward passes.  Holds where every kept pt
    is a normal number of the dtype, which the oracle is asked first: scores within a few hundredths of each other."""
    D = 8
    _, cases = F.layouts(dtype, H, D)
    case = cases[0]
    if mode == 'dot':
        sr, sc, v, _ = _operands(mode, case, dtype, H, D, 600, 0)
        scalar = 0.1 * D ** -0.5
    else:
        sr, sc, v, _ = _operands(mode, case, dtype, H, D, 600, 0, spread=0.05)
        scalar = 0.2
    rate, seed = 0.6, 4242
    drop = (rate, seed)
    plain, ex = _oracle(mode, case, dtype, None, sr, sc, v, scalar, drop)
    keep, c = R.keep_mask(seed, rate, case.E, H), R.scale_of(rate)
    out, lse = F.store(ex.out, dtype), ex.lse.astype(F.ACC[dtype])
    go = F.store(np.random.default_rng(601).standard_normal(ex.out.shape), dtype)
    nsr, nsc, nv, no, ng = _numbers(dtype, sr, sc, v, out, go)
    expect = R.bw_exact(mode, case.ptr, case.ind, None, nsr, nsc, nv, no, lse.astype(np.float64), ng, scalar, keep, c, dtype)
    assert float(expect[0][keep].min()) > 2 * R.SMALLEST_NORMAL[dtype], 'every kept pt is a normal number'
    assert bool((expect[0][~keep] == 0).all())
    pt, d = call_bw(dev, mode, dtype, case, None, sr, sc, v, out, lse, go, scalar, drop, with_row=H == 1)
    assert np.array_equal(F.numbers(pt, dtype) != 0, keep)
    R.check_bw(pt, d, expect, dtype)


# ---- 5: C-ABI backward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('dtype', F.FLOATS)
def test_cabi_backward_pt_and_d(dev, mode, dtype):
    """pt and ds / dz from the oracle's out and lse (stored), on a layout of three wave windows: row given and searched,
    packets and generic, every bias form, -inf entries exact zeros, a row of -inf only NaN."""
    case = F.edge_case(64 * 2 + 9, nsrc=23)
    lens = np.diff(case.ptr)
    worst, n = (0.0, 0.0), 0
    for H, D in ((1, 1), (2, 3), (3, 8), (8, 16), (2, 128), (20, 4)):
        form = n % 3
        sr, sc, v, bias = _operands(mode, case, dtype, H, D, 700 + n, form)
        if bias is not None:
            nb = F.numbers(bias, dtype)
            long_row = int(np.argmax(lens))
            nb[case.ptr[long_row]] = -np.inf
            dead = int(np.nonzero((lens >= 2) & (np.arange(lens.size) != long_row))[0][0])
            nb[case.ptr[dead]:case.ptr[dead + 1]] = -np.inf
            bias = F.store(nb, dtype)
        scalar = ((D ** -0.5, 0.37, -1.5) if mode == 'dot' else (0.2, 1.0, 0.05))[n % 3]
        drop = ((0.6, 31 + n), (0.1, 2 ** 40 + n))[n % 2]
        n += 1
        plain, ex = _oracle(mode, case, dtype, bias, sr, sc, v, scalar, drop)
        keep, c = R.keep_mask(drop[1], drop[0], case.E, H), R.scale_of(drop[0])
        out, lse = F.store(ex.out, dtype), ex.lse.astype(F.ACC[dtype])
        go = F.store(np.random.default_rng(701 + n).standard_normal(ex.out.shape), dtype)
        nsr, nsc, nv, nb, no, ng = _numbers(dtype, sr, sc, v, bias, out, go)
        expect = R.bw_exact(mode, case.ptr, case.ind, nb, nsr, nsc, nv, no, lse.astype(np.float64), ng, scalar, keep, c, dtype)
        if bias is not None:
            assert np.isnan(expect[0]).any() and bool((expect[0][keep] == 0).any())
        for off in (0, 8):
            pt, d = call_bw(dev, mode, dtype, case, bias, sr, sc, v, out, lse, go, scalar, drop, with_row=off == 0, off=off)
            pt2, d2 = call_bw(dev, mode, dtype, case, bias, sr, sc, v, out, lse, go, scalar, drop, with_row=off != 0, off=off)
            assert _same(pt, pt2) and _same(d, d2), 'row given and row searched differ'
            try:
                w = R.check_bw(pt, d, expect, dtype)
            except AssertionError as exc:
                raise AssertionError('%s: %s' % ((H, D, off), exc)) from None
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print('%s %s dropout backward: worst err / bound pt %.3g d %.3g' % ((mode, dtype) + worst))


# ---- 6: degenerate shapes and status codes -----------------------------------------------------------------------------
@pytest.mark.parametrize('mode', R.MODES)
def test_cabi_degenerate_shapes_and_status_codes(dev, mode):
    L = nat.lib()
    fake = ctypes.c_void_p(0x1000)
    stream = nat.stream_ptr(dev)
    sz = ctypes.c_size_t
    fw, bw = getattr(L, FW[mode][1]), getattr(L, BW[mode][1])
    OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
    names = [L.tsamd_status_string(i).decode().lower() for i in range(5)]
    assert 'invalid' in names[INVALID] and 'support' in names[UNSUPPORTED] and 'workspace' in names[WORKSPACE], names

    def f(rate=0.5, dtype=0, bias=None, bh=1, sr=fake, out=fake, lse=fake, M=4, N=4, H=2, D=3, E=5, ws=fake, nws=1 << 20,
          rowptr=fake):
        return fw(dtype, rowptr, fake, bias, bh, sr, fake, fake, 1.0, rate, 9, out, lse, M, N, H, D, E, ws, sz(nws), stream)

    def b(rate=0.5, dtype=0, bias=None, bh=1, row=None, rowptr=fake, p=fake, M=4, N=4, H=2, D=3, E=5):
        return bw(dtype, row, rowptr, fake, bias, bh, fake, fake, fake, fake, fake, fake, 1.0, rate, 9, p, fake, M, N, H, D, E,
                  stream)

    # the rate comes first: before a negative size, an unsupported dtype, and the shapes that are TSAMD_OK without work
    for rate in (float('nan'), -0.5, 1.0, 2.0, float('inf')):
        for call in (f, b):
            assert call(rate=rate) == INVALID
            assert call(rate=rate, M=-1) == INVALID and call(rate=rate, dtype=5) == INVALID
            assert call(rate=rate, E=0) == INVALID and call(rate=rate, H=0) == INVALID
    # then the twin's cases in the twin's order
    for call in (f, b):
        assert call(M=-1, dtype=5) == INVALID and call(dtype=5) == UNSUPPORTED
        assert call(N=1 << 31) == UNSUPPORTED
        assert call(dtype=5, bias=fake, bh=3) == UNSUPPORTED and call(bias=fake, bh=3) == INVALID
    for M, H, D in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        assert f(M=M, H=H, D=D, out=None, lse=None, ws=None, nws=0) == OK
    assert f(out=None) == INVALID and f(lse=None) == INVALID
    assert f(sr=None) == INVALID and f(N=0) == INVALID and f(rowptr=None) == INVALID
    assert f(ws=None) == WORKSPACE and f(nws=8) == WORKSPACE
    for E, H in ((0, 2), (5, 0)):
        assert b(E=E, H=H, p=None) == OK
    assert b(D=0) == INVALID and b(p=None) == INVALID and b(M=0) == INVALID and b(N=0) == INVALID
    assert b(row=None, rowptr=None) == INVALID
    # E = 0: zeros and -inf, nothing else read
    out = torch.full((4, 2, 3), 7.0, device=dev)
    lse = torch.full((4, 2), 7.0, device=dev)
    with torch.cuda.device(dev):
        assert fw(0, None, None, None, 1, None, None, None, 1.0, 0.6, 1, nat._ptr(out), nat._ptr(lse), 4, 4, 2, 3, 0, None,
                  sz(0), stream) == OK
    assert bool((out == 0).all()) and bool(torch.isneginf(lse).all())
    op = torch.ops.tsamd.attention_heads if mode == 'dot' else torch.ops.tsamd.gat_attention_heads
    ptr0 = torch.zeros(5, dtype=torch.int64, device=dev)
    col0 = torch.zeros(0, dtype=torch.int64, device=dev)
    srs = torch.ones((4, 2, 3) if mode == 'dot' else (4, 2), device=dev)
    scs = torch.ones((6, 2, 3) if mode == 'dot' else (6, 2), device=dev)
    o, l = op(ptr0, col0, None, srs, scs, torch.ones(6, 2, 3, device=dev), 1.0, 0.6, 3)
    assert o.shape == (4, 2, 3) and bool((o == 0).all()) and bool(torch.isneginf(l).all())


# ---- 7: the public calls ---------------------------------------------------------------------------------------------
def _pattern():
    """300 x 200, rows 7..11 and columns 50..59 empty, row 123 a hub that holds every other column."""
    rng = np.random.default_rng(12)
    mask = rng.random((300, 200)) < 0.04
    mask[123] = True
    mask[7:12] = False
    mask[:, 50:60] = False
    row, col = np.nonzero(mask)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=300))]).astype(np.int64)
    return mask, row.astype(np.int64), col.astype(np.int64), F.Case('pattern', ptr, col.astype(np.int64), row.size, 300, 200)


@pytest.fixture(scope='module')
def pattern():
    return _pattern()


def _adj(ts, dev, case, value=None):
    row = F._seg_of(case.ptr, case.nseg, case.E)
    return ts.SparseTensor(row=torch.from_numpy(row).to(dev), col=torch.from_numpy(case.ind).to(dev), value=value,
                           sparse_sizes=(case.nseg, case.nsrc), is_sorted=True)


def _public(A, mode, sr, sc, v, scalar, bias=False, **kw):
    return (A.attention if mode == 'dot' else A.gat_attention)(sr, sc, v, scalar, bias, **kw)


def _t(a, dtype, dev):
    return None if a is None else fromnp(np.ascontiguousarray(a), TORCH[dtype]).to(dev)


@pytest.mark.parametrize('mode', R.MODES)
def test_public_call_against_dense_fp64_with_the_oracles_mask(ts, dev, pattern, mode):
    mask, row, col, case = pattern
    H, D, E = 3, 5, case.E
    rng = np.random.default_rng(800)
    rate, seed = 0.6, 2 ** 62 + 5
    keep, c = R.keep_mask(seed, rate, E, H), R.scale_of(rate)
    for form in (0, 1, 2):
        sr = torch.from_numpy(rng.standard_normal((300, H, D) if mode == 'dot' else (300, H)))
        sc = torch.from_numpy(rng.standard_normal((200, H, D) if mode == 'dot' else (200, H)))
        v = torch.from_numpy(rng.standard_normal((200, H, D)))
        go = torch.from_numpy(rng.standard_normal((300, H, D)))
        bias = (None, torch.from_numpy(rng.standard_normal(E)), torch.from_numpy(rng.standard_normal((E, H))))[form]
        cpu = [t.clone().requires_grad_() for t in (sr, sc, v)] + ([bias.clone().requires_grad_()] if form else [])
        want = R.dense_torch(mode, mask, row, col, cpu[3] if form else None, cpu[0], cpu[1], cpu[2], SCALAR[mode], keep, c)
        wg = torch.autograd.grad(want, cpu, go)
        gl = [t.to(dev).requires_grad_() for t in (sr, sc, v)] + ([bias.to(dev).requires_grad_()] if form else [])
        A = _adj(ts, dev, case, value=gl[3] if form else None)
        out = _public(A, mode, gl[0], gl[1], gl[2], SCALAR[mode], bool(form), dropout=rate, seed=seed)
        assert out.requires_grad and out.dtype == torch.float64
        assert torch.allclose(out.detach().cpu(), want.detach(), rtol=1e-11, atol=1e-13) and bool((out[7:12] == 0).all())
        for g, w, name in zip(torch.autograd.grad(out, gl, go.to(dev)), wg, ('sr', 'sc', 'v', 'bias')):
            assert g.shape == w.shape and torch.allclose(g.cpu(), w, rtol=1e-9, atol=1e-12), (form, name)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_public_call_and_all_gradients_inside_the_bounds(ts, dev, mode, dtype):
    """On the hub layout (M != N): out inside the bound of the oracle, the four gradients inside the bound of the oracle's,
    which is given the forward's own out and lse as the backward kernel is."""
    H, D = 3, 8
    _, cases = F.layouts(dtype, H, D)
    case = cases[0]
    rate, seed = 0.6, 31337
    keep, c = R.keep_mask(seed, rate, case.E, H), R.scale_of(rate)
    for form in (2, 1, 0):
        sr, sc, v, bias = _operands(mode, case, dtype, H, D, 810 + form, form)
        nsr, nsc, nv, nb = _numbers(dtype, sr, sc, v, bias)
        _, ex = _oracle(mode, case, dtype, bias, sr, sc, v, SCALAR[mode], (rate, seed))
        leaves = [_t(a, dtype, dev).requires_grad_() for a in (sr, sc, v)]
        tb = None if form == 0 else _t(bias, dtype, dev).requires_grad_()
        A = _adj(ts, dev, case, value=tb)
        out = _public(A, mode, leaves[0], leaves[1], leaves[2], SCALAR[mode], form != 0, dropout=rate, seed=seed)
        rowptr, col, _ = A.csr()
        op = torch.ops.tsamd.attention_heads if mode == 'dot' else torch.ops.tsamd.gat_attention_heads
        o2, lse = op(rowptr, col, None if tb is None else tb.detach(), *[t.detach() for t in leaves], SCALAR[mode], rate, seed)
        assert bits_equal(o2, out.detach()) and lse.dtype == ACC_T[dtype]
        ra = R.check(mode, tonp(out.detach()), tonp(lse), ex, dtype)
        go = F.store(np.random.default_rng(820 + form).standard_normal(ex.out.shape), dtype)
        got = torch.autograd.grad(out, leaves + ([tb] if form else []), _t(go, dtype, dev))
        expect = R.grads_exact(mode, case.ptr, case.ind, nb, nsr, nsc, nv, SCALAR[mode], F.numbers(go, dtype), keep, c, dtype,
                               out=F.numbers(tonp(o2), dtype), lse=tonp(lse).astype(np.float64))
        got = R.Grads(*[tonp(g) for g in got], *([] if form else [None]))
        rg = R.check_grads(got, expect, dtype, shared_bias=form == 1)
        print('%s %s form %d: worst err / bound out %.3g lse %.3g, gradients (sr, sc, v, bias) %s'
              % (mode, dtype, form, ra[0], ra[1], ' '.join('%.3g' % x for x in rg)))


def _tiny():
    rng = np.random.default_rng(160)
    mask = rng.random((12, 9)) < 0.35
    mask[4] = False
    mask[:, 2] = False
    row, col = np.nonzero(mask)
    ptr = np.zeros(13, np.int64)
    np.cumsum(np.bincount(row, minlength=12), out=ptr[1:])
    return mask, F.Case('tiny', ptr, col.astype(np.int64), row.size, 12, 9)


def test_gradcheck_with_a_fixed_seed(ts, dev):
    mask, case = _tiny()
    A = _adj(ts, dev, case)
    rng = np.random.default_rng(830)
    q, k, v, b2 = (torch.from_numpy(rng.standard_normal(s)).to(dev).requires_grad_()
                   for s in ((12, 2, 3), (9, 2, 3), (9, 2, 3), (case.E, 2)))
    assert torch.autograd.gradcheck(lambda a, b, c: A.attention(a, b, c, 0.8, dropout=0.5, seed=5), (q, k, v), nondet_tol=0.0)
    fn = lambda a, b, c, d: A.set_value(d, layout='coo').attention(a, b, c, bias=True, dropout=0.3, seed=6)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (q, k, v, b2), nondet_tol=0.0)
    a_dst, a_src, x, b1, _ = (torch.from_numpy(a).to(dev).requires_grad_()
                              for a in G.gradcheck_operands(case.ptr, case.ind, 12, 9, 2, 3, seed=160))
    assert torch.autograd.gradcheck(lambda a, b, c: A.gat_attention(a, b, c, 0.2, dropout=0.5, seed=5), (a_dst, a_src, x),
                                    nondet_tol=0.0)
    fn = lambda a, b, c, d: A.set_value(d, layout='coo').gat_attention(a, b, c, 0.3, bias=True, dropout=0.6, seed=7)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (a_dst, a_src, x, b1), nondet_tol=0.0)


@pytest.mark.parametrize('mode', R.MODES)
def test_seeds_training_flag_and_flat_operands(ts, dev, pattern, mode):
    mask, row, col, case = pattern
    H, D = 2, 6
    rng = np.random.default_rng(840)
    sr = torch.from_numpy(rng.standard_normal((300, H, D) if mode == 'dot' else (300, H))).float().to(dev)
    sc = torch.from_numpy(rng.standard_normal((200, H, D) if mode == 'dot' else (200, H))).float().to(dev)
    v = torch.from_numpy(rng.standard_normal((200, H, D))).float().to(dev)
    A = _adj(ts, dev, case)
    call = lambda **kw: _public(A, mode, sr, sc, v, SCALAR[mode], **kw)  # noqa: E731
    plain = call()
    # the same seed gives the same bits, also through the function of the package and with gradients
    a, b = call(dropout=0.6, seed=9), call(dropout=0.6, seed=9)
    assert bits_equal(a, b) and not bits_equal(a, plain) and not bits_equal(a, call(dropout=0.6, seed=10))
    fn = ts.attention if mode == 'dot' else ts.gat_attention
    assert bits_equal(a, fn(A, sr, sc, v, SCALAR[mode], False, 0.6, True, 9))
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_() for t in (sr, sc, v)]
        out = _public(A, mode, *leaves, SCALAR[mode], dropout=0.6, seed=9)
        runs.append([out.detach()] + list(torch.autograd.grad(out, leaves, torch.ones_like(out))))
    assert all(bits_equal(x, y) for x, y in zip(*runs)) and bits_equal(runs[0][0], a)
    # seed=None draws host_seed() from torch's CPU generator: reproducible, a new one per call
    torch.manual_seed(3)
    c1, c2 = call(dropout=0.6), call(dropout=0.6)
    assert bits_equal(c1, call(dropout=0.6, seed=npd.host_seed(3))) and not bits_equal(c1, c2)
    torch.manual_seed(3)
    assert bits_equal(c1, call(dropout=0.6))
    # nothing dropped: today's call bit for bit, and torch's generator left alone
    state = torch.get_rng_state()
    assert bits_equal(plain, call(dropout=0.6, training=False)) and bits_equal(plain, call(dropout=0.0))
    assert bits_equal(plain, call(dropout=0.0, seed=4)) and bits_equal(plain, call(dropout=0.6, training=False, seed=4))
    assert torch.equal(state, torch.get_rng_state())
    # the expectation is the plain call: the mean over seeds moves towards it
    mean = torch.stack([call(dropout=0.5, seed=s) for s in range(64)]).mean(0)
    assert float((mean - plain).abs().mean()) < 0.5 * float((a - plain).abs().mean())
    # one head as 2-D operands
    flat = _public(A, mode, sr[:, 0], sc[:, 0], v[:, 0], SCALAR[mode], dropout=0.6, seed=9)
    want = _public(A, mode, sr[:, :1], sc[:, :1], v[:, :1], SCALAR[mode], dropout=0.6, seed=9)
    assert flat.shape == (300, D) and bits_equal(flat, want[:, 0])
    g = [t.clone().requires_grad_() for t in (sr[:, 0], sc[:, 0], v[:, 0])]
    _public(A, mode, *g, SCALAR[mode], dropout=0.6, seed=9).sum().backward()
    assert all(t.grad.shape == t.shape for t in g)


@pytest.mark.parametrize('mode', R.MODES)
def test_only_the_gradients_asked_for_build_the_column_caches(ts, dev, pattern, mode):
    mask, row, col, case = pattern
    H, D = 2, 4
    rng = np.random.default_rng(850)
    sr, sc, v, b = (torch.from_numpy(rng.standard_normal(s)).to(dev)
                    for s in ((300, H, D) if mode == 'dot' else (300, H), (200, H, D) if mode == 'dot' else (200, H),
                              (200, H, D), (case.E, H)))

    def run(which):
        t = {n: a.clone().requires_grad_(n in which) for n, a in (('r', sr), ('c', sc), ('v', v), ('b', b))}
        A = _adj(ts, dev, case, value=t['b'])
        _public(A, mode, t['r'], t['c'], t['v'], SCALAR[mode], True, dropout=0.6, seed=1).sum().backward()
        assert [n for n in t if t[n].grad is not None] == list(which)
        return A.storage._colptr is None and A.storage._csr2csc is None

    assert run('r') and run('b') and run('rb'), 'no column-side gradient: the CSC caches stay None'
    assert not run('c') and not run('v') and not run('rcvb')


def test_scripted_module_calls_the_extended_operators(ts, dev, pattern):
    class Layer(torch.nn.Module):
        def forward(self, rowptr: torch.Tensor, col: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    a_dst: torch.Tensor, a_src: torch.Tensor, go: torch.Tensor, rate: float, seed: int):
            out, lse = torch.ops.tsamd.attention_heads(rowptr, col, None, q, k, v, 0.35, rate, seed)
            p, ds = torch.ops.tsamd.attention_heads_bw(None, rowptr, col, None, q, k, v, out, lse, go, 0.35, rate, seed)
            out2, lse2 = torch.ops.tsamd.gat_attention_heads(rowptr, col, None, a_dst, a_src, v, 0.2, rate, seed)
            p2, dz = torch.ops.tsamd.gat_attention_heads_bw(None, rowptr, col, None, a_dst, a_src, v, out2, lse2, go, 0.2,
                                                            dropout=rate, seed=seed)
            old, _ = torch.ops.tsamd.attention_heads(rowptr, col, None, q, k, v, 0.35)  # the positional callers of before
            return out, p, ds, out2, p2, dz, old

    mask, row, col, case = pattern
    rng = np.random.default_rng(860)
    q, k, v, go = (torch.from_numpy(rng.standard_normal(s)).float().to(dev)
                   for s in ((300, 2, 8), (200, 2, 8), (200, 2, 8), (300, 2, 8)))
    a_dst, a_src = (torch.from_numpy(rng.standard_normal(s)).float().to(dev) for s in ((300, 2), (200, 2)))
    A = _adj(ts, dev, case)
    rowptr, colidx, _ = A.csr()
    got = torch.jit.script(Layer())(rowptr, colidx, q, k, v, a_dst, a_src, go, 0.6, 77)
    for a, b in zip(got, Layer()(rowptr, colidx, q, k, v, a_dst, a_src, go, 0.6, 77)):
        assert bits_equal(a, b)
    assert bits_equal(got[0], A.attention(q, k, v, 0.35, dropout=0.6, seed=77))
    assert bits_equal(got[3], A.gat_attention(a_dst, a_src, v, 0.2, dropout=0.6, seed=77))
    assert bits_equal(got[6], A.attention(q, k, v, 0.35))
    keep = torch.from_numpy(R.keep_mask(77, 0.6, case.E, 2)).to(dev)
    assert torch.equal(got[1] != 0, keep) and torch.equal(got[4] != 0, keep)


def test_errors(ts, dev, pattern):
    mask, row, col, case = pattern
    A = _adj(ts, dev, case)
    f = lambda *s: torch.ones(*s, device=dev)  # noqa: E731
    dot = lambda **kw: A.attention(f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), **kw)  # noqa: E731
    gat = lambda **kw: A.gat_attention(f(300, 2), f(200, 2), f(200, 2, 4), **kw)  # noqa: E731
    for call in (dot, gat):
        for rate in (1.0, -0.1, 1.5, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='dropout'):
                call(dropout=rate)
            with pytest.raises(ValueError, match='dropout'):
                call(dropout=rate, training=False)
        for seed in (-1, 2 ** 63):
            with pytest.raises(ValueError, match='seed'):
                call(dropout=0.5, seed=seed)
        for seed in (1.0, '1', torch.tensor(1), True):
            with pytest.raises(TypeError, match='seed'):
                call(dropout=0.5, seed=seed)
        with pytest.raises(TypeError, match='dropout'):
            call(dropout='0.5')
        assert call(dropout=0.5, seed=2 ** 63 - 1).shape == (300, 2, 4)
    rowptr, colidx, _ = A.csr()
    for op, args in ((torch.ops.tsamd.attention_heads, (f(300, 2, 4), f(200, 2, 4), f(200, 2, 4))),
                     (torch.ops.tsamd.gat_attention_heads, (f(300, 2), f(200, 2), f(200, 2, 4)))):
        for rate in (1.0, -0.1, float('nan')):
            with pytest.raises(RuntimeError, match='dropout'):
                op(rowptr, colidx, None, *args, 0.5, rate, 0)
        with pytest.raises(RuntimeError, match='seed'):
            op(rowptr, colidx, None, *args, 0.5, 0.5, -1)
    out, lse = torch.ops.tsamd.attention_heads(rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), 1.0, 0.5, 3)
    with pytest.raises(RuntimeError, match='dropout'):
        torch.ops.tsamd.attention_heads_bw(None, rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), out, lse,
                                           f(300, 2, 4), 1.0, 1.0, 3)
    with pytest.raises(RuntimeError, match='seed'):
        torch.ops.tsamd.gat_attention_heads_bw(None, rowptr, colidx, None, f(300, 2), f(200, 2), f(200, 2, 4), out, lse,
                                               f(300, 2, 4), 0.2, 0.5, -3)
