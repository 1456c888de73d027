"""The additive score mode of csrc/attention.hip against tests/gat_attention_reference.py: the forward through the C entry
point on every shape, alignment, bias form, slope and census layout, non-finite values, degenerate shapes, the backward
kernel's p and dz, and the operators / SparseTensor.gat_attention against the fp64 oracle, the library chain, the
oracle's gradients, dense fp64 autograd and gradcheck.  Every operand set is built by G.operands, which asserts its
census on the host (tests/test_gat_attention_reference.py asserts it for all of them without a device)."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import fused_attention_reference as F
from tests import gat_attention_reference as G
from tests.util import bits_equal, fromnp, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
ACC_T = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float32, 'bf16': torch.float32}
HEADS = (1, 2, 3, 8)
FEATS = (1, 3, 4, 8, 16, 24, 64)
SLOPES = (0.2, 0.0, 1.0)
GUARD = 64  # elements before and after an output that no call may touch


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


def call_fw(dev, dtype, case, ops, slope, off=0, fill_ws=85):
    """tsamd_gat_attention_heads through ctypes into guarded, pre-filled out and lse over a sentinel-filled workspace; v
    and out at `off` modulo 16, a_dst and a_src one element off the boundary when v is on it -> (out, lse)."""
    tdt, adt = TORCH[dtype], ACC_T[dtype]
    M, H = ops.a_dst.shape
    N, D = ops.v.shape[0], ops.v.shape[2]
    aoff = tdt.itemsize if off == 0 else 0
    dd, ds = _place(ops.a_dst, tdt, dev, aoff), _place(ops.a_src, tdt, dev, aoff)
    dv = _place(ops.v, tdt, dev, off)
    db = None if ops.bias is None else _place(ops.bias, tdt, dev, 0)
    dptr, dind = _dev(case.ptr, dev), _dev(case.ind, dev)
    L = nat.lib()
    nbytes = L.tsamd_attention_heads_workspace_bytes(F.CODE[dtype], H, D, case.E)
    assert nbytes == F.workspace_bytes(dtype, H, D, case.E)
    ws = nat.workspace(nbytes, dev)
    ws.fill_(fill_ws)  # whatever an earlier call left there must not matter
    raw, start, out = _guarded(M * H * D, tdt, dev, off)
    lraw, lstart, lse = _guarded(M * H, adt, dev, 0)
    with torch.cuda.device(dev):
        st = L.tsamd_gat_attention_heads(F.CODE[dtype], nat._ptr(dptr), nat._ptr(dind), nat._ptr(db),
                                         1 if ops.bias is None or ops.bias.ndim == 1 else H, nat._ptr(dd), nat._ptr(ds),
                                         nat._ptr(dv), float(slope), out, lse, M, N, H, D, case.E, nat._ptr(ws),
                                         ctypes.c_size_t(nbytes), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_gat_attention_heads')
    return tonp(_read(raw, start, (M, H, D), tdt)), tonp(_read(lraw, lstart, (M, H), adt))


def _same(a, b):
    return F.same_bits(np.asarray(a), np.asarray(b))


def _exact(case, ops, slope, dtype):
    return G.exact(case.ptr, case.ind, *[G.numbers(a, dtype) for a in (ops.bias, ops.a_dst, ops.a_src, ops.v)], slope)


def _run_and_check(dev, dtype, case, ops, slope, offs=(0, ), ex=None):
    """Both fills of the workspace give the same bits; inside the bound -> (ratio out, ratio lse)."""
    if ex is None:
        ex = _exact(case, ops, slope, dtype)
    worst = (0.0, 0.0)
    for off in offs:
        out, lse = call_fw(dev, dtype, case, ops, slope, off=off, fill_ws=85)
        out2, lse2 = call_fw(dev, dtype, case, ops, slope, off=off, fill_ws=0)
        assert _same(out, out2) and _same(lse, lse2), 'two calls differ'
        empty = np.diff(case.ptr) == 0
        assert bool((F.numbers(out, dtype)[empty] == 0).all()) and bool(np.isneginf(lse[empty]).all())
        r = G.check(out, lse, ex, dtype)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    return worst


# ---- C-ABI forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', G.FLOATS)
def test_cabi_forward_every_shape_alignment_bias_and_slope(dev, dtype):
    """H x D x alignment on the hub layout of that shape's chunk length (census asserted): rows inside a chunk, cut once,
    spanning three chunks and more, empty leading and trailing rows, a tile boundary; no bias, [nnz] and [nnz, H]; the
    slopes 0.2, 0 and 1; a_dst / a_src one element off the boundary on the packet route."""
    sets = G.gpu_sets('shape', dtype)
    assert [(s.H, s.D) for s in sets] == [(H, D) for H in HEADS for D in FEATS]
    worst, routes = (0.0, 0.0), set()
    for n, s in enumerate(sets):
        H, D, form = s.H, s.D, s.form
        r, case, ops = G.build(s)
        assert case.name == 'hub'
        for off in (0, 8):
            got = (ctypes.c_int64 * 8)()
            f = F.AR._fake(off == 0)
            assert nat.lib().tsamd_attention_heads_route(F.CODE[dtype], H, D, None, None, f, f, got) == 0
            got = F.AtRoute(*[int(x) for x in got])
            assert got == F.expected_route(dtype, H, D, off == 0) and got.chunk == r.chunk
            routes.add(got.generic)
        try:
            w = _run_and_check(dev, dtype, case, ops, SLOPES[(n // 3) % 3], offs=(0, 8))
        except AssertionError as exc:
            raise AssertionError('%s: %s' % ((H, D, form), exc)) from None
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    assert routes == {0, 1}
    print('%s additive forward: worst err / bound out %.3g lse %.3g' % ((dtype, ) + worst))


@pytest.mark.parametrize('dtype,D', [('f32', 264), ('bf16', 520)])
def test_cabi_forward_head_wider_than_a_wave(dev, dtype, D):
    """D above 64 lanes' worth of features: every feature block of the head forms the score itself."""
    H = 1
    for aligned in (True, False):
        r = F.route(dtype, H, D, aligned)
        assert r.fblocks == 2 and r.blocks == 2 and r.lanes_per_head == 64 and r.generic == (0 if aligned else 1)
    (s, ) = [s for s in G.gpu_sets('wide', dtype) if s.D == D]
    r, case, ops = G.build(s)
    w = _run_and_check(dev, dtype, case, ops, 0.2, offs=(0, 8))
    print('%s wide head: worst err / bound out %.3g lse %.3g' % ((dtype, ) + w))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_cabi_forward_every_layout_peak_and_large_scores(dev, dtype):
    """The census layouts (hub, more rows in a tile than LDS holds, a single source row) under every slope; the hub with
    its maximum in the first chunk, the last, and both; scores beyond +-80."""
    worst = (0.0, 0.0)
    for s in G.gpu_sets('layout', dtype):
        r, case, ops = G.build(s)
        for slope in SLOPES:
            try:
                w = _run_and_check(dev, dtype, case, ops, slope)
            except AssertionError as exc:
                raise AssertionError('%s slope %s: %s' % (case.name, slope, exc)) from None
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    assert case.name == 'one_source' and case.nsrc == 1
    peaks = G.gpu_sets('peak', dtype)
    assert [s.peak for s in peaks] == list(G.PEAKS)
    for s in peaks:
        r, hub, ops = G.build(s)
        w = _run_and_check(dev, dtype, hub, ops, 0.2)
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    r, hub, ops = G.build(G.gpu_sets('large', dtype)[0])
    for slope in (1.0, 0.2):
        ex = _exact(hub, ops, slope, dtype)
        assert float(ex.s.max()) > 80 and (slope != 1.0 or float(ex.s.min()) < -80)
        w = _run_and_check(dev, dtype, hub, ops, slope, ex=ex)
    print('%s layouts: worst err / bound out %.3g lse %.3g; scores to +-%.0f: %.3g %.3g'
          % ((dtype, ) + worst + (float(np.abs(ex.s).max()), ) + w))


def test_a_nan_in_a_src_poisons_the_rows_and_the_head_that_touch_it(dev):
    H, D, dtype = 3, 8, 'f32'
    r, case, ops = G.build(G.gpu_sets('nan')[0])
    hub = int(np.argmax(np.diff(case.ptr)))
    row = F._seg_of(case.ptr, case.nseg, case.E)
    clean_out, clean_lse = call_fw(dev, dtype, case, ops, 0.2)
    assert np.isfinite(clean_out).all() and np.isfinite(clean_lse[np.diff(case.ptr) > 0]).all()
    for bad in (float('nan'), float('inf')):
        a_src = ops.a_src.copy()
        a_src[5, 2] = bad  # every row that gathers column 5, head 2 -- the hub among them
        out, lse = call_fw(dev, dtype, case, ops._replace(a_src=a_src), 0.2)
        want = np.zeros((case.nseg, H), bool)
        want[np.unique(row[case.ind == 5]), 2] = True
        assert want[hub, 2], 'the hub gathers column 5: its neighbours of length 0 and 1 share its chunk and its records'
        assert np.array_equal(np.isnan(lse), want) and np.array_equal(np.isnan(out), np.repeat(want[:, :, None], D, 2))
        assert _same(out[~want], clean_out[~want]) and _same(lse[~want], clean_lse[~want]), 'nothing else moved'
        assert want.any(1).sum() < case.nseg - 10, 'most rows stay finite'
    a_dst = ops.a_dst.copy()
    a_dst[hub + 2, 1] = float('nan')  # a row of one entry beside the hub, head 1
    out, lse = call_fw(dev, dtype, case, ops._replace(a_dst=a_dst), 0.2)
    want = np.zeros((case.nseg, H), bool)
    want[hub + 2, 1] = True
    assert np.array_equal(np.isnan(lse), want) and _same(out[~want], clean_out[~want])


def test_minus_inf_bias_masks_entries_and_a_row_of_them_is_nan(dev):
    H, D, dtype = 3, 8, 'f32'
    r, case, ops = G.build(G.gpu_sets('minus_inf')[0])
    lens = np.diff(case.ptr)
    hub = int(np.argmax(lens))
    cut = int(np.nonzero(lens == 7)[0][-1])
    clean_out, clean_lse = call_fw(dev, dtype, case, ops, 0.2)
    bias = ops.bias.copy()
    lo, hi = int(case.ptr[hub]), int(case.ptr[hub + 1])
    bias[lo:hi:3, 0] = -np.inf                                  # every third entry of the hub, head 0
    bias[lo:lo + r.chunk + 3, 2] = -np.inf                      # its whole first piece and more, head 2
    bias[case.ptr[cut]:case.ptr[cut + 1], 1] = -np.inf          # a whole row, head 1
    masked = ops._replace(bias=bias)
    out, lse = call_fw(dev, dtype, case, masked, 0.2)
    G.check(out, lse, _exact(case, masked, 0.2, dtype), dtype)
    assert np.isnan(out[cut, 1]).all() and np.isneginf(lse[cut, 1]) and np.isfinite(out[hub]).all()
    moved = np.zeros((case.nseg, H), bool)
    moved[hub, 0] = moved[hub, 2] = moved[cut, 1] = True
    assert _same(out[~moved], clean_out[~moved]) and _same(lse[~moved], clean_lse[~moved]), 'nothing else moved'
    # slope 0: 0 * -inf is NaN, the mask is lost and the row is NaN (documented, not special-cased)
    out, lse = call_fw(dev, dtype, case, masked, 0.0)
    G.check(out, lse, _exact(case, masked, 0.0, dtype), dtype)
    assert np.isnan(out[hub, 0]).all() and np.isnan(lse[hub, 0]) and np.isfinite(out[hub, 1]).all()


def test_cabi_degenerate_shapes(dev):
    L = nat.lib()
    fake = ctypes.c_void_p(0x1000)
    stream = nat.stream_ptr(dev)
    sz = ctypes.c_size_t
    OK, INVALID = 0, 1
    for M, H, D in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        assert L.tsamd_gat_attention_heads(0, fake, fake, None, 1, fake, fake, fake, 0.2, None, None, M, 4, H, D, 5, None,
                                           sz(0), stream) == OK
    for E, H in ((0, 2), (5, 0)):
        assert L.tsamd_gat_attention_heads_bw(0, None, fake, fake, None, 1, fake, fake, fake, fake, fake, fake, 0.2, fake,
                                              fake, 4, 4, H, 3, E, stream) == OK
    assert L.tsamd_gat_attention_heads(0, fake, fake, None, 1, fake, fake, fake, 0.2, fake, fake, 4, 0, 2, 3, 5, fake,
                                       sz(1 << 20), stream) == INVALID, 'entries without a source row'
    assert L.tsamd_gat_attention_heads_bw(0, None, fake, fake, None, 1, fake, fake, fake, fake, fake, fake, 0.2, fake,
                                          fake, 4, 0, 2, 3, 5, stream) == INVALID
    # E = 0 and rows that are all empty: zeros and -inf, nothing else read
    out = torch.full((4, 2, 3), 7.0, device=dev)
    lse = torch.full((4, 2), 7.0, device=dev)
    with torch.cuda.device(dev):
        assert L.tsamd_gat_attention_heads(0, None, None, None, 1, None, None, None, 0.2, nat._ptr(out), nat._ptr(lse), 4,
                                           4, 2, 3, 0, None, sz(0), stream) == OK
    assert bool((out == 0).all()) and bool(torch.isneginf(lse).all())
    A = torch.ops.tsamd.gat_attention_heads
    ptr0 = torch.zeros(5, dtype=torch.int64, device=dev)
    col0 = torch.zeros(0, dtype=torch.int64, device=dev)
    o, l = A(ptr0, col0, None, torch.ones(4, 2, device=dev), torch.ones(6, 2, device=dev), torch.ones(6, 2, 3, device=dev),
             0.2)
    assert o.shape == (4, 2, 3) and bool((o == 0).all()) and bool(torch.isneginf(l).all())
    o, l = A(torch.zeros(1, dtype=torch.int64, device=dev), col0, None, torch.ones(0, 2, device=dev),
             torch.ones(6, 2, device=dev), torch.ones(6, 2, 3, device=dev), 0.2)
    assert o.shape == (0, 2, 3) and l.shape == (0, 2)
    o, l = A(ptr0, col0, None, torch.ones(4, 0, device=dev), torch.ones(6, 0, device=dev), torch.ones(6, 0, 3, device=dev),
             0.2)
    assert o.shape == (4, 0, 3) and l.shape == (4, 0)


# ---- C-ABI backward kernel ------------------------------------------------------------------------------------------------
def call_bw(dev, dtype, case, ops, out, lse, go, slope, with_row, off=0):
    tdt, adt = TORCH[dtype], ACC_T[dtype]
    M, H = ops.a_dst.shape
    N, D = ops.v.shape[0], ops.v.shape[2]
    aoff = tdt.itemsize if off == 0 else 0
    dd, ds_ = _place(ops.a_dst, tdt, dev, aoff), _place(ops.a_src, tdt, dev, aoff)
    dv, do, dg = (_place(a, tdt, dev, off) for a in (ops.v, out, go))
    db = None if ops.bias is None else _place(ops.bias, tdt, dev, 0)
    dl = _place(lse, adt, dev, 0)
    row = F._seg_of(case.ptr, M, case.E) if with_row else None
    dptr, dind, drow = (_dev(a, dev) for a in (case.ptr, case.ind, row))
    praw, pstart, p = _guarded(case.E * H, tdt, dev, 0)
    zraw, zstart, dz = _guarded(case.E * H, tdt, dev, 0)
    with torch.cuda.device(dev):
        st = nat.lib().tsamd_gat_attention_heads_bw(F.CODE[dtype], nat._ptr(drow), nat._ptr(dptr), nat._ptr(dind),
                                                    nat._ptr(db), 1 if ops.bias is None or ops.bias.ndim == 1 else H,
                                                    nat._ptr(dd), nat._ptr(ds_), nat._ptr(dv), nat._ptr(do), nat._ptr(dl),
                                                    nat._ptr(dg), float(slope), p, dz, M, N, H, D, case.E,
                                                    nat.stream_ptr(dev))
    nat.check(st, 'tsamd_gat_attention_heads_bw')
    return tonp(_read(praw, pstart, (case.E, H), tdt)), tonp(_read(zraw, zstart, (case.E, H), tdt))


@pytest.mark.parametrize('dtype', G.FLOATS)
def test_cabi_backward_p_and_dz(dev, dtype):
    """p and dz from the forward's own out and lse, on census layouts: row given and searched, both routes, every bias
    form and slope, the entry with z == 0, -inf entries exact zeros, a row of -inf only NaN."""
    worst = (0.0, 0.0)
    for n, s in enumerate(G.gpu_sets('backward', dtype)):
        H, D, form = s.H, s.D, s.form
        r, case, ops = G.build(s)
        lens = np.diff(case.ptr)
        if form:
            nb = G.numbers(ops.bias, dtype)
            long_row = int(np.argmax(lens))
            nb[case.ptr[long_row]] = -np.inf                    # one masked entry (every head it covers)
            dead = int(np.nonzero((lens >= 2) & (np.arange(lens.size) != long_row))[0][0])
            nb[case.ptr[dead]:case.ptr[dead + 1]] = -np.inf     # a row of -inf only
            ops = ops._replace(bias=G.store(nb, dtype))
        slope = SLOPES[n] if not form else 0.2                  # a -inf bias masks only under a positive slope
        out, lse = call_fw(dev, dtype, case, ops, slope)
        go = G.store(np.random.default_rng(133 + n).standard_normal(out.shape), dtype)
        num = [G.numbers(a, dtype) for a in (ops.bias, ops.a_dst, ops.a_src, ops.v)]
        expect = G.bw_exact(case.ptr, case.ind, *num, G.numbers(out, dtype), lse.astype(np.float64), G.numbers(go, dtype),
                            slope, dtype)
        assert bool((G.preact(case.ptr, case.ind, *num[:3])[0] == 0).any())
        if form:
            assert np.isnan(expect[0]).any() and bool((expect[0] == 0).any())
        for off in (0, 8):
            p, dz = call_bw(dev, dtype, case, ops, out, lse, go, slope, with_row=off == 0, off=off)
            p2, dz2 = call_bw(dev, dtype, case, ops, out, lse, go, slope, with_row=off != 0, off=off)
            assert _same(p, p2) and _same(dz, dz2), 'row given and row searched differ'
            try:
                w = G.check_bw(p, dz, expect, dtype)
            except AssertionError as exc:
                raise AssertionError('%s: %s' % ((H, D, off), exc)) from None
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print('%s additive backward: worst err / bound p %.3g dz %.3g' % ((dtype, ) + worst))


# ---- operators and the Python surface ----------------------------------------------------------------------------------
def _adj(ts, dev, case, value=None):
    row = F._seg_of(case.ptr, case.nseg, case.E)
    return ts.SparseTensor(row=torch.from_numpy(row).to(dev), col=torch.from_numpy(case.ind).to(dev), value=value,
                           sparse_sizes=(case.nseg, case.nsrc), is_sorted=True)


def _t(a, dtype, dev):
    return None if a is None else fromnp(np.ascontiguousarray(a), TORCH[dtype]).to(dev)


def _chain(A, a_dst, a_src, v, slope, bias):
    row, col, _ = A.coo()
    z = a_dst[row] + a_src[col]
    if bias is not None:
        z = z + (bias if bias.dim() == 2 else bias[:, None])
    return A.set_value(torch.nn.functional.leaky_relu(z, slope), 'coo').softmax(1).matmul_heads(v)


@pytest.mark.parametrize('dtype', G.FLOATS)
def test_public_call_and_all_gradients_against_the_oracle(ts, dev, dtype):
    """SparseTensor.gat_attention on the hub layout (M != N) in every dtype: out inside the bound of the fp64 oracle, as
    is the library chain in float32 / float64 (in the 16-bit types the chain stores its scores rounded to 16 bits: that
    is the chain's error, not the bound's); the four gradients inside the bound of the oracle's, which is given the
    forward's own out and lse as the backward kernel is."""
    for s, slope in zip(G.gpu_sets('public', dtype), (0.2, 0.2, 1.0)):
        H, D, form = s.H, s.D, s.form
        r, case, ops = G.build(s)
        assert case.nseg != case.nsrc
        num = [G.numbers(a, dtype) for a in (ops.bias, ops.a_dst, ops.a_src, ops.v)]
        ex = G.exact(case.ptr, case.ind, *num, slope)
        leaves = [_t(a, dtype, dev).requires_grad_() for a in (ops.a_dst, ops.a_src, ops.v)]
        tb = None if form == 0 else _t(ops.bias, dtype, dev).requires_grad_()
        A = _adj(ts, dev, case, value=tb)
        assert A.storage._colptr is None and A.storage._csr2csc is None
        out = A.gat_attention(leaves[0], leaves[1], leaves[2], slope, bias=form != 0)
        assert out.shape == (case.nseg, H, D) and out.dtype == TORCH[dtype] and out.requires_grad
        rowptr, col, _ = A.csr()
        o2, lse = torch.ops.tsamd.gat_attention_heads(rowptr, col, None if tb is None else tb.detach(),
                                                      *[t.detach() for t in leaves], slope)
        assert bits_equal(o2, out.detach()) and lse.shape == (case.nseg, H) and lse.dtype == ACC_T[dtype]
        assert bits_equal(out.detach(), ts.gat_attention(A, *[t.detach() for t in leaves], slope, form != 0))
        ra = G.check(tonp(out.detach()), tonp(lse), ex, dtype)
        if dtype in ('f32', 'f64'):
            with torch.no_grad():
                chain = _chain(A, *[t.detach() for t in leaves], slope, None if tb is None else tb.detach())
            bo, _ = G.bounds(ex, dtype)
            rb = F._ratio(tonp(chain).astype(np.float64), ex.out, bo, 'chain', dtype)
            print('%s form %d: worst err / bound fused out %.3g lse %.3g, chain %.3g' % (dtype, form, ra[0], ra[1], rb))
        go = G.store(np.random.default_rng(140 + form).standard_normal(ex.out.shape), dtype)
        got = torch.autograd.grad(out, leaves + ([tb] if form else []), _t(go, dtype, dev))
        expect = G.grads_exact(case.ptr, case.ind, *num, slope, G.numbers(go, dtype), dtype,
                               G.numbers(tonp(o2), dtype), tonp(lse).astype(np.float64))
        got = G.Grads(*[tonp(g) for g in got], *([] if form else [None]))
        assert got.a_dst.shape == ops.a_dst.shape and got.a_src.shape == ops.a_src.shape and got.v.shape == ops.v.shape
        assert form == 0 or got.bias.shape == ops.bias.shape
        rg = G.check_grads(got, expect, dtype, shared_bias=form == 1)
        print('%s form %d gradients (a_dst, a_src, v, bias): worst err / bound %s' % (dtype, form, ' '.join('%.3g' % x for x in rg)))


def _tiny():
    rng = np.random.default_rng(160)
    mask = rng.random((12, 9)) < 0.35
    mask[4] = False
    mask[:, 2] = False
    row, col = np.nonzero(mask)
    ptr = np.zeros(13, np.int64)
    np.cumsum(np.bincount(row, minlength=12), out=ptr[1:])
    return mask, F.Case('tiny', ptr, col.astype(np.int64), row.size, 12, 9)


def test_gradients_against_dense_fp64_autograd_and_gradcheck(ts, dev):
    mask, case = _tiny()
    row = F._seg_of(case.ptr, case.nseg, case.E)
    a_dst, a_src, v, b1, b2 = (torch.from_numpy(a) for a in G.gradcheck_operands(case.ptr, case.ind, 12, 9, 2, 3, seed=160))
    A = _adj(ts, dev, case)
    for slope in (0.2, 0.0, -0.5):
        for bias in (None, b1, b2):
            cpu = [t.clone().requires_grad_() for t in (a_dst, a_src, v)] + ([bias.clone().requires_grad_()] if bias is not None else [])
            z = cpu[0][:, None, :] + cpu[1][None, :, :]
            if bias is not None:
                b = cpu[3] if bias.dim() == 2 else cpu[3][:, None].expand(-1, 2)
                z = z + torch.zeros_like(z).index_put((torch.from_numpy(row), torch.from_numpy(case.ind)), b)
            s = torch.nn.functional.leaky_relu(z, slope)
            m3 = torch.from_numpy(mask)[:, :, None].expand_as(s)
            P = torch.softmax(torch.where(m3, s, torch.full_like(s, -np.inf)), 1)
            P = torch.where(m3 & ~torch.isnan(P), P, torch.zeros_like(P))
            want = torch.einsum('mnh,nhd->mhd', P, cpu[2])
            go = torch.from_numpy(np.random.default_rng(161).standard_normal(want.shape))
            wg = torch.autograd.grad(want, cpu, go)
            gl = [t.to(dev).requires_grad_() for t in (a_dst, a_src, v)] + ([bias.to(dev).requires_grad_()] if bias is not None else [])
            Ab = A if bias is None else A.set_value(gl[3], layout='coo')
            out = Ab.gat_attention(gl[0], gl[1], gl[2], slope, bias=bias is not None)
            assert torch.allclose(out.detach().cpu(), want.detach(), rtol=1e-11, atol=1e-13) and bool((out[4] == 0).all())
            for g, w in zip(torch.autograd.grad(out, gl, go.to(dev)), wg):
                assert g.shape == w.shape and torch.allclose(g.cpu(), w, rtol=1e-9, atol=1e-12)
    q, k, x, c1, c2 = (t.to(dev).requires_grad_() for t in (a_dst, a_src, v, b1, b2))
    assert torch.autograd.gradcheck(lambda a, b, c: A.gat_attention(a, b, c, 0.2), (q, k, x), nondet_tol=0.0)
    for bias in (c1, c2):
        fn = lambda a, b, c, d: A.set_value(d, layout='coo').gat_attention(a, b, c, 0.3, bias=True)  # noqa: E731
        assert torch.autograd.gradcheck(fn, (q, k, x, bias), nondet_tol=0.0)
    y = A.gat_attention(q, k, x)
    gq, = torch.autograd.grad((y * y).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):  # no second order
        gq.sum().backward()


def test_one_dimensional_operands_expanded_grad_out_and_determinism(ts, dev):
    dtype, H, D = 'f32', 1, 6
    r, case, ops = G.build(G.gpu_sets('flat')[0])
    A = _adj(ts, dev, case)
    a_dst, a_src, v = (_t(a, dtype, dev) for a in (ops.a_dst, ops.a_src, ops.v))
    flat = A.gat_attention(a_dst[:, 0], a_src[:, 0], v[:, 0])
    assert flat.shape == (case.nseg, D) and bits_equal(flat, A.gat_attention(a_dst, a_src, v, 0.2)[:, 0])
    assert not bits_equal(flat, A.gat_attention(a_dst[:, 0], a_src[:, 0], v[:, 0], 0.5))
    g = [t.clone().requires_grad_() for t in (a_dst[:, 0], a_src[:, 0], v[:, 0])]
    A.gat_attention(*g).sum().backward()  # an expanded grad_out
    assert all(t.grad.shape == t.shape for t in g)
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            leaves = [t.clone().requires_grad_() for t in (a_dst, a_src, v)]
            out = A.gat_attention(*leaves)
            runs.append([out.detach()] + list(torch.autograd.grad(out, leaves, torch.ones(1, 1, 1, device=dev).expand_as(out))))
        for a, b in zip(*runs):
            assert bits_equal(a, b), 'two calls differ'
        for a, b in zip(runs[0][1:], (t.grad for t in g)):
            assert bits_equal(a[:, 0] if a.dim() > b.dim() else a, b), 'the expanded gradient is the contiguous one'
    finally:
        torch.use_deterministic_algorithms(before)


def test_only_the_gradients_asked_for_and_the_column_caches(ts, dev):
    dtype = 'f32'
    r, case, ops = G.build(G.gpu_sets('caches')[0])
    a_dst, a_src, v, b = (_t(a, dtype, dev) for a in (ops.a_dst, ops.a_src, ops.v, ops.bias))

    def run(which):
        t = {n: a.clone().requires_grad_(n in which) for n, a in (('d', a_dst), ('s', a_src), ('v', v), ('b', b))}
        A = _adj(ts, dev, case, value=t['b'])
        A.gat_attention(t['d'], t['s'], t['v'], bias=True).sum().backward()
        assert [n for n in t if t[n].grad is not None] == list(which)
        return A.storage._colptr is None and A.storage._csr2csc is None

    assert run('d') and run('b') and run('db'), 'no column-side gradient: the CSC caches stay None'
    assert not run('s') and not run('v') and not run('dsvb')
    A = _adj(ts, dev, case)
    with torch.no_grad():
        A.gat_attention(a_dst.clone().requires_grad_(), a_src.clone().requires_grad_(), v.clone().requires_grad_())
    assert A.storage._colptr is None and A.storage._csr2csc is None


def test_scripted_module_calls_the_operators(ts, dev):
    class Layer(torch.nn.Module):
        def forward(self, rowptr: torch.Tensor, col: torch.Tensor, a_dst: torch.Tensor, a_src: torch.Tensor,
                    v: torch.Tensor, go: torch.Tensor, slope: float):
            out, lse = torch.ops.tsamd.gat_attention_heads(rowptr, col, None, a_dst, a_src, v, slope)
            p, dz = torch.ops.tsamd.gat_attention_heads_bw(None, rowptr, col, None, a_dst, a_src, v, out, lse, go, slope)
            return out, p, dz

    dtype, H, D = 'f32', 3, 8
    r, case, ops = G.build(G.gpu_sets('script')[0])
    a_dst, a_src, v = (_t(a, dtype, dev) for a in (ops.a_dst, ops.a_src, ops.v))
    go = torch.randn(case.nseg, H, D, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    A = _adj(ts, dev, case)
    rowptr, col, _ = A.csr()
    got = torch.jit.script(Layer())(rowptr, col, a_dst, a_src, v, go, 0.2)
    for a, b in zip(got, Layer()(rowptr, col, a_dst, a_src, v, go, 0.2)):
        assert bits_equal(a, b)
    assert bits_equal(got[0], A.gat_attention(a_dst, a_src, v, 0.2))
    sums = torch.zeros(case.nseg, H, device=dev).index_add_(0, A.storage.row(), got[1])
    nonempty = (rowptr[1:] > rowptr[:-1])
    assert torch.allclose(sums[nonempty], torch.ones_like(sums[nonempty]), atol=1e-5), 'the probabilities of a row add to 1'


def test_errors(ts, dev):
    _, case = _tiny()
    A = _adj(ts, dev, case)
    M, N, E = case.nseg, case.nsrc, case.E
    f = lambda *s: torch.ones(*s, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match='heads'):
        A.gat_attention(f(M, 2), f(N, 3), f(N, 3, 4))
    with pytest.raises(ValueError, match='heads'):
        A.gat_attention(f(M, 2), f(N, 2), f(N, 3, 4))
    with pytest.raises(ValueError, match='dimensions'):
        A.gat_attention(f(M, 2), f(N, 2), f(N, 8))
    with pytest.raises(ValueError, match='dimensions'):
        A.gat_attention(f(M), f(N), f(N, 1, 8))
    with pytest.raises(ValueError, match='floating'):
        A.gat_attention(f(M, 2).long(), f(N, 2).long(), f(N, 2, 4).long())
    with pytest.raises(ValueError, match='dtype'):
        A.gat_attention(f(M, 2), f(N, 2), f(N, 2, 4).double())
    with pytest.raises(ValueError, match='rows'):
        A.gat_attention(f(M - 1, 2), f(N, 2), f(N, 2, 4))
    with pytest.raises(ValueError, match='columns'):
        A.gat_attention(f(M, 2), f(N - 1, 2), f(N, 2, 4))
    with pytest.raises(ValueError, match='columns'):
        A.gat_attention(f(M, 2), f(N, 2), f(N - 1, 2, 4))
    with pytest.raises(ValueError, match='at least one feature'):
        A.gat_attention(f(M, 2), f(N, 2), f(N, 2, 0))
    with pytest.raises(ValueError, match='finite'):
        A.gat_attention(f(M, 2), f(N, 2), f(N, 2, 4), float('nan'))
    with pytest.raises(TypeError, match='Tensor'):
        A.gat_attention(f(M, 2), None, f(N, 2, 4))
    with pytest.raises(ValueError, match='values'):
        A.gat_attention(f(M, 2), f(N, 2), f(N, 2, 4), bias=True)
    with pytest.raises(ValueError, match='bias'):
        A.set_value(f(E, 3), layout='coo').gat_attention(f(M, 2), f(N, 2), f(N, 2, 4), bias=True)
    with pytest.raises(ValueError, match='floating'):
        A.set_value(f(E).long(), layout='coo').gat_attention(f(M, 2), f(N, 2), f(N, 2, 4), bias=True)
    with pytest.raises(RuntimeError, match='GPU'):
        A.gat_attention(torch.ones(M, 2), torch.ones(N, 2), torch.ones(N, 2, 4))
    rowptr, colidx, _ = A.csr()
    op = torch.ops.tsamd.gat_attention_heads
    with pytest.raises(RuntimeError, match='heads'):
        op(rowptr, colidx, None, f(M, 2), f(N, 3), f(N, 3, 4), 0.2)
    with pytest.raises(RuntimeError, match='heads'):
        op(rowptr, colidx, None, f(M, 2), f(N, 2), f(N, 3, 4), 0.2)
    with pytest.raises(RuntimeError, match='rows'):
        op(rowptr, colidx, None, f(M, 2), f(N - 1, 2), f(N, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='dimension'):
        op(rowptr, colidx, None, f(M), f(N, 2), f(N, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='entries'):
        op(rowptr, colidx, f(E - 1), f(M, 2), f(N, 2), f(N, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='heads'):
        op(rowptr, colidx, f(E, 3), f(M, 2), f(N, 2), f(N, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='float32, float64, float16 or bfloat16'):
        op(rowptr, colidx, None, f(M, 2).long(), f(N, 2).long(), f(N, 2, 4).long(), 0.2)
    with pytest.raises(RuntimeError, match='dtype'):
        op(rowptr, colidx, None, f(M, 2), f(N, 2).double(), f(N, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='rowptr'):
        op(rowptr[:-1], colidx, None, f(M, 2), f(N, 2), f(N, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='finite'):
        op(rowptr, colidx, None, f(M, 2), f(N, 2), f(N, 2, 4), float('inf'))
    out, lse = op(rowptr, colidx, None, f(M, 2), f(N, 2), f(N, 2, 4), 0.2)
    bwop = torch.ops.tsamd.gat_attention_heads_bw
    with pytest.raises(RuntimeError, match='lse'):
        bwop(None, rowptr, colidx, None, f(M, 2), f(N, 2), f(N, 2, 4), out, lse.double(), f(M, 2, 4), 0.2)
    with pytest.raises(RuntimeError, match='grad_out'):
        bwop(None, rowptr, colidx, None, f(M, 2), f(N, 2), f(N, 2, 4), out, lse, f(M, 2, 5), 0.2)
    with pytest.raises(RuntimeError, match='out must be'):
        bwop(None, rowptr, colidx, None, f(M, 2), f(N, 2), f(N, 2, 4), out[:-1], lse, f(M, 2, 4), 0.2)
