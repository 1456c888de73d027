"""csrc/attention.hip against tests/fused_attention_reference.py: the forward through the C entry point on every shape,
alignment, bias form and layout (route and census asserted on the host first), rows of one entry, degenerate shapes,
non-finite values, the backward kernel's p and ds, and the operators / SparseTensor.attention against dense fp64 torch,
the three-step chain, fp64 autograd and gradcheck."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import attention_reference as AR
from tests import fused_attention_reference as F
from tests.util import bits_equal, fromnp, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
ACC_T = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float32, 'bf16': torch.float32}
HEADS = (1, 2, 3, 8)
FEATS = (1, 3, 4, 8, 16, 24, 64, 128)
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


def call_fw(dev, dtype, case, bias, q, k, v, scale, off=0, fill_ws=85):
    """tsamd_attention_heads through ctypes into guarded, pre-filled out and lse over a sentinel-filled workspace ->
    (out [M, H, D] stored elements, lse [M, H])."""
    tdt, adt = TORCH[dtype], ACC_T[dtype]
    M, H, D = q.shape
    dq, dk, dv = (_place(a, tdt, dev, off) for a in (q, k, v))
    db = None if bias is None else _place(bias, tdt, dev, 0)
    dptr, dind = _dev(case.ptr, dev), _dev(case.ind, dev)
    L = nat.lib()
    nbytes = L.tsamd_attention_heads_workspace_bytes(F.CODE[dtype], H, D, case.E)
    assert nbytes == F.workspace_bytes(dtype, H, D, case.E)
    ws = nat.workspace(nbytes, dev)
    ws.fill_(fill_ws)  # whatever an earlier call left there must not matter
    raw, start, out = _guarded(M * H * D, tdt, dev, off)
    lraw, lstart, lse = _guarded(M * H, adt, dev, 0)
    with torch.cuda.device(dev):
        st = L.tsamd_attention_heads(F.CODE[dtype], nat._ptr(dptr), nat._ptr(dind), nat._ptr(db),
                                     1 if bias is None or bias.ndim == 1 else H, nat._ptr(dq), nat._ptr(dk), nat._ptr(dv),
                                     float(scale), out, lse, M, k.shape[0], H, D, case.E, nat._ptr(ws),
                                     ctypes.c_size_t(nbytes), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_attention_heads')
    return tonp(_read(raw, start, (M, H, D), tdt)), tonp(_read(lraw, lstart, (M, H), adt))


def _bias(case, dtype, H, form, seed):
    rng = np.random.default_rng(seed)
    if form == 0:
        return None
    return F.store(rng.standard_normal(case.E if form == 1 else (case.E, H)), dtype)


def _same(a, b):
    return F.same_bits(np.asarray(a), np.asarray(b))


def _run_and_check(dev, dtype, case, bias, q, k, v, scale, offs=(0, ), ex=None):
    """Both fills of the workspace give the same bits; inside the bound -> (ratio out, ratio lse)."""
    if ex is None:
        ex = F.exact(case.ptr, case.ind, F.numbers(bias, dtype), F.numbers(q, dtype), F.numbers(k, dtype),
                     F.numbers(v, dtype), scale)
    worst = (0.0, 0.0)
    for off in offs:
        out, lse = call_fw(dev, dtype, case, bias, q, k, v, scale, off=off, fill_ws=85)
        out2, lse2 = call_fw(dev, dtype, case, bias, q, k, v, scale, off=off, fill_ws=0)
        assert _same(out, out2) and _same(lse, lse2), 'two calls differ'
        empty = np.diff(case.ptr) == 0
        assert bool((F.numbers(out, dtype)[empty] == 0).all()) and bool(np.isneginf(lse[empty]).all())
        r = F.check(out, lse, ex, dtype)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    return worst


# ---- C-ABI forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', F.FLOATS)
def test_cabi_forward_every_shape_alignment_and_bias(dev, dtype):
    """H x D x alignment on the hub layout of that shape's chunk length (census asserted): rows inside a chunk, cut once,
    spanning three chunks and more, empty leading and trailing rows, a tile boundary; no bias, [nnz] and [nnz, H]."""
    worst, routes, n = (0.0, 0.0), set(), 0
    for H in HEADS:
        for D in FEATS:
            r = F.route(dtype, H, D)
            case = F.hub_case(r.chunk, r.tile)
            c = F.census(case, r.chunk, r.tile, r.tile)
            assert c['span3'] >= 1 and c['cut'] >= 1 and c['inside'] >= 3 and c['empty'] >= 6, c
            q, k, v = F.operands(case, dtype, H, D, seed=60 + n)
            bias = _bias(case, dtype, H, n % 3, 61 + n)
            scale = (D ** -0.5, 0.37, -1.5)[n % 3]
            n += 1
            for off in (0, 8):
                got = F.route(dtype, H, D, off == 0)
                assert got == F.expected_route(dtype, H, D, off == 0) and got.chunk == r.chunk
                routes.add(got.generic)
            try:
                w = _run_and_check(dev, dtype, case, bias, q, k, v, scale, offs=(0, 8))
            except AssertionError as exc:
                raise AssertionError('%s: %s' % ((H, D, n % 3), exc)) from None
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    assert routes == {0, 1}
    print('%s fused forward: worst err / bound out %.3g lse %.3g' % ((dtype, ) + worst))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_cabi_forward_head_wider_than_a_wave(dev, dtype):
    """D above 64 lanes' worth of features: the feature blocks of a head each form the whole score."""
    H, D = 2, 300 if dtype == 'f32' else 150
    for aligned in (True, False):
        r = F.route(dtype, H, D, aligned)
        assert r.fblocks == 2 and r.blocks == 4 and r.lanes_per_head == 64 and r.generic == (0 if aligned else 1)
    case = F.hub_case(r.chunk, r.tile)
    q, k, v = F.operands(case, dtype, H, D, seed=70)
    w = _run_and_check(dev, dtype, case, _bias(case, dtype, H, 2, 71), q, k, v, D ** -0.5, offs=(0, 8))
    print('%s wide head: worst err / bound out %.3g lse %.3g' % ((dtype, ) + w))


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_cabi_forward_every_tile_edge_and_layout(dev, dtype):
    """E = 1 and every window / chunk / wave / tile size minus one, exact, plus one; the census layouts (hub, more rows in
    a tile than LDS holds, a single source row); the hub with its maximum in the first chunk, the last, and both; scores
    near +-80."""
    H, D = 3, 8
    r, census = F.layouts(dtype, H, D)
    sizes = F.edge_sizes(r.chunk, r.chunk // 8, 512, r.tile)
    assert 1 in sizes and r.chunk + 1 in sizes and r.tile - 1 in sizes and 513 in sizes
    cases = [F.edge_case(E) for E in sizes] + census
    worst = (0.0, 0.0)
    for i, case in enumerate(cases):
        q, k, v = F.operands(case, dtype, H, D, seed=80 + i)
        try:
            w = _run_and_check(dev, dtype, case, _bias(case, dtype, H, i % 3, 81 + i), q, k, v, 0.5)
        except AssertionError as exc:
            raise AssertionError('%s: %s' % (case.name, exc)) from None
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    hub = census[0]
    for where in F.PEAKS:
        q, k, v = F.operands(hub, dtype, H, D, seed=90)
        bias = F.store(F.peak_bias(hub, r.chunk, where), dtype)
        w = _run_and_check(dev, dtype, hub, bias, q, k, v, 0.5)
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    q, k, v = F.operands(hub, dtype, H, D, seed=91, spread=30.0)
    ex = F.exact(hub.ptr, hub.ind, None, F.numbers(q, dtype), F.numbers(k, dtype), F.numbers(v, dtype), 0.5)
    assert float(np.abs(ex.s).max()) > 80
    w = _run_and_check(dev, dtype, hub, None, q, k, v, 0.5, ex=ex)
    print('%s layouts: worst err / bound out %.3g lse %.3g; scores to +-%.0f: %.3g %.3g'
          % ((dtype, ) + worst + (float(np.abs(ex.s).max()), ) + w))


@pytest.mark.parametrize('dtype', F.FLOATS)
def test_row_of_one_entry_returns_its_value_row(dev, dtype):
    H, D = 3, 8
    rng = np.random.default_rng(100)
    lens = [1, 0, 1, 1, 0, 0] * 40 + [1]
    case = AR._case('ones', lens, 19, rng)
    q, k, v = F.operands(case, dtype, H, D, seed=101)
    out, lse = call_fw(dev, dtype, case, None, q, k, v, 0.4)
    rows = np.nonzero(np.diff(case.ptr) == 1)[0]
    assert _same(out[rows], v[case.ind]), 'softmax of one entry is 1: the value row, bit for bit'
    score = AR.sddmm_exact(case.ptr, case.ind, None, F.numbers(q, dtype), F.numbers(k, dtype), 0.4)
    AR.check(lse[rows].astype(F.ACC[dtype]), score, 'f64' if dtype == 'f64' else 'f32')  # lse is the score, rounded once


def test_cabi_degenerate_shapes(dev):
    L = nat.lib()
    fake = ctypes.c_void_p(0x1000)
    stream = nat.stream_ptr(dev)
    sz = ctypes.c_size_t
    for M, H, D in ((0, 2, 3), (4, 0, 3), (4, 2, 0)):
        assert L.tsamd_attention_heads(0, fake, fake, None, 1, fake, fake, fake, 1.0, None, None, M, 4, H, D, 5, None,
                                       sz(0), stream) == 0
    for E, H in ((0, 2), (5, 0)):
        assert L.tsamd_attention_heads_bw(0, None, fake, fake, None, 1, fake, fake, fake, fake, fake, fake, 1.0, fake,
                                          fake, 4, 4, H, 3, E, stream) == 0
    # E = 0 and rows that are all empty: zeros and -inf, nothing else read
    out = torch.full((4, 2, 3), 7.0, device=dev)
    lse = torch.full((4, 2), 7.0, device=dev)
    with torch.cuda.device(dev):
        assert L.tsamd_attention_heads(0, None, None, None, 1, None, None, None, 1.0, nat._ptr(out), nat._ptr(lse), 4, 4,
                                       2, 3, 0, None, sz(0), stream) == 0
    assert bool((out == 0).all()) and bool(torch.isneginf(lse).all())
    A = torch.ops.tsamd.attention_heads
    ptr0 = torch.zeros(5, dtype=torch.int64, device=dev)
    col0 = torch.zeros(0, dtype=torch.int64, device=dev)
    o, l = A(ptr0, col0, None, torch.ones(4, 2, 3, device=dev), torch.ones(6, 2, 3, device=dev),
             torch.ones(6, 2, 3, device=dev), 1.0)
    assert o.shape == (4, 2, 3) and bool((o == 0).all()) and bool(torch.isneginf(l).all())
    o, l = A(torch.zeros(1, dtype=torch.int64, device=dev), col0, None, torch.ones(0, 2, 3, device=dev),
             torch.ones(6, 2, 3, device=dev), torch.ones(6, 2, 3, device=dev), 1.0)
    assert o.shape == (0, 2, 3) and l.shape == (0, 2)
    o, l = A(ptr0, col0, None, torch.ones(4, 0, 3, device=dev), torch.ones(6, 0, 3, device=dev),
             torch.ones(6, 0, 3, device=dev), 1.0)
    assert o.shape == (4, 0, 3) and l.shape == (4, 0)


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_non_finite_inputs_stay_in_their_row_and_head(dev, bad):
    H, D, dtype = 3, 8, 'f32'
    r = F.route(dtype, H, D)
    case = F.hub_case(r.chunk, r.tile)
    q, k, v = F.operands(case, dtype, H, D, seed=110)
    q, k = np.abs(q) + 0.5, np.abs(k) + 0.5  # no 0 * inf, no inf - inf: the poisoned outputs are known by position
    hub = int(np.argmax(np.diff(case.ptr)))
    row = F._seg_of(case.ptr, case.nseg, case.E)
    one = hub + 2
    assert case.ptr[one + 1] - case.ptr[one] == 1
    clean_out, clean_lse = call_fw(dev, dtype, case, None, q, k, v, 0.3)
    assert np.isfinite(clean_out).all() and np.isfinite(clean_lse[np.diff(case.ptr) > 0]).all()
    q2, k2, v2 = q.copy(), k.copy(), v.copy()
    q2[one, 1, 3] = bad   # a row of one entry beside the hub, head 1
    k2[5, 2, 0] = bad     # every row that gathers column 5, head 2 -- the hub among them
    out, lse = call_fw(dev, dtype, case, None, q2, k2, v, 0.3)
    want = np.zeros((case.nseg, H), bool)
    want[one, 1] = True
    want[np.unique(row[case.ind == 5]), 2] = True
    assert want[hub, 2], 'the hub gathers column 5: its neighbours of length 0 and 1 share its chunk and its records'
    assert np.array_equal(np.isnan(lse), want) and np.array_equal(np.isnan(out), np.repeat(want[:, :, None], D, 2))
    assert _same(out[~want], clean_out[~want]) and _same(lse[~want], clean_lse[~want]), 'nothing else moved'
    assert want.any(1).sum() < case.nseg - 10, 'most rows stay finite'
    v2[7, 0, 1] = bad     # one feature of a value row: that feature of the rows that gather it
    out, lse = call_fw(dev, dtype, case, None, q, k, v2, 0.3)
    wantv = np.zeros((case.nseg, H, D), bool)
    wantv[np.unique(row[case.ind == 7]), 0, 1] = True
    assert np.array_equal(~np.isfinite(out), wantv) and _same(out[~wantv], clean_out[~wantv]) and _same(lse, clean_lse)


def test_minus_inf_bias_masks_entries_and_a_row_of_them_is_nan(dev):
    H, D, dtype = 3, 8, 'f32'
    r = F.route(dtype, H, D)
    case = F.hub_case(r.chunk, r.tile)
    q, k, v = F.operands(case, dtype, H, D, seed=120)
    lens = np.diff(case.ptr)
    hub = int(np.argmax(lens))
    cut = int(np.nonzero(lens == 7)[0][-1])
    zero = np.zeros((case.E, H), np.float32)
    clean_out, clean_lse = call_fw(dev, dtype, case, zero, q, k, v, 0.3)
    bias = zero.copy()
    lo, hi = int(case.ptr[hub]), int(case.ptr[hub + 1])
    bias[lo:hi:3, 0] = -np.inf                                  # every third entry of the hub, head 0
    bias[lo:lo + r.chunk + 3, 2] = -np.inf                      # its whole first piece and more, head 2
    bias[case.ptr[cut]:case.ptr[cut + 1], 1] = -np.inf          # a whole row, head 1
    out, lse = call_fw(dev, dtype, case, bias, q, k, v, 0.3)
    ex = F.exact(case.ptr, case.ind, bias, q, k, v, 0.3)
    F.check(out, lse, ex, dtype)
    assert np.isnan(out[cut, 1]).all() and np.isneginf(lse[cut, 1]) and np.isfinite(out[hub]).all()
    moved = np.zeros((case.nseg, H), bool)
    moved[hub, 0] = moved[hub, 2] = moved[cut, 1] = True
    assert _same(out[~moved], clean_out[~moved]) and _same(lse[~moved], clean_lse[~moved]), 'nothing else moved'


# ---- C-ABI backward kernel ------------------------------------------------------------------------------------------------
def call_bw(dev, dtype, case, bias, q, k, v, out, lse, go, scale, with_row, off=0):
    tdt, adt = TORCH[dtype], ACC_T[dtype]
    M, H, D = q.shape
    dq, dk, dv, do, dg = (_place(a, tdt, dev, off) for a in (q, k, v, out, go))
    db = None if bias is None else _place(bias, tdt, dev, 0)
    dl = _place(lse, adt, dev, 0)
    row = F._seg_of(case.ptr, M, case.E) if with_row else None
    dptr, dind, drow = (_dev(a, dev) for a in (case.ptr, case.ind, row))
    praw, pstart, p = _guarded(case.E * H, tdt, dev, 0)
    sraw, sstart, ds = _guarded(case.E * H, tdt, dev, 0)
    with torch.cuda.device(dev):
        st = nat.lib().tsamd_attention_heads_bw(F.CODE[dtype], nat._ptr(drow), nat._ptr(dptr), nat._ptr(dind), nat._ptr(db),
                                                1 if bias is None or bias.ndim == 1 else H, nat._ptr(dq), nat._ptr(dk),
                                                nat._ptr(dv), nat._ptr(do), nat._ptr(dl), nat._ptr(dg), float(scale), p, ds,
                                                M, k.shape[0], H, D, case.E, nat.stream_ptr(dev))
    nat.check(st, 'tsamd_attention_heads_bw')
    return tonp(_read(praw, pstart, (case.E, H), tdt)), tonp(_read(sraw, sstart, (case.E, H), tdt))


@pytest.mark.parametrize('dtype', F.FLOATS)
def test_cabi_backward_p_and_ds(dev, dtype):
    """p and ds from the oracle's out and lse (stored), on a layout of three wave windows: row given and searched, both
    routes, every bias form, -inf entries exact zeros, a row of -inf only NaN."""
    case = F.edge_case(64 * 2 + 9, nsrc=23)
    lens = np.diff(case.ptr)
    worst, n = (0.0, 0.0), 0
    for H, D in ((1, 1), (2, 3), (3, 8), (8, 16), (3, 24), (2, 128), (20, 4), (1, 600)):
        q, k, v = F.operands(case, dtype, H, D, seed=130 + n)
        bias = _bias(case, dtype, H, n % 3, 131 + n)
        if bias is not None:
            nb = F.numbers(bias, dtype)
            long_row = int(np.argmax(lens))
            nb[case.ptr[long_row]] = -np.inf                    # one masked entry (every head it covers)
            dead = int(np.nonzero((lens >= 2) & (np.arange(lens.size) != long_row))[0][0])
            nb[case.ptr[dead]:case.ptr[dead + 1]] = -np.inf     # a row of -inf only
            bias = F.store(nb, dtype)
        scale = (D ** -0.5, 0.37, -1.5)[n % 3]
        n += 1
        nq, nk, nv, nb = (F.numbers(a, dtype) for a in (q, k, v, bias))
        ex = F.exact(case.ptr, case.ind, nb, nq, nk, nv, scale)
        out = F.store(ex.out, dtype)
        lse = ex.lse.astype(F.ACC[dtype])
        go = F.store(np.random.default_rng(132 + n).standard_normal(q.shape), dtype)
        expect = F.bw_exact(case.ptr, case.ind, nb, nq, nk, nv, F.numbers(out, dtype), lse.astype(np.float64),
                            F.numbers(go, dtype), scale)
        if bias is not None:
            assert np.isnan(expect[0]).any() and bool((expect[0] == 0).any())
        for off in (0, 8):
            p, ds = call_bw(dev, dtype, case, bias, q, k, v, out, lse, go, scale, with_row=off == 0, off=off)
            p2, ds2 = call_bw(dev, dtype, case, bias, q, k, v, out, lse, go, scale, with_row=off != 0, off=off)
            assert _same(p, p2) and _same(ds, ds2), 'row given and row searched differ'
            try:
                w = F.check_bw(p, ds, expect, dtype)
            except AssertionError as exc:
                raise AssertionError('%s: %s' % ((H, D, off), exc)) from None
            worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print('%s fused backward: worst err / bound p %.3g ds %.3g' % ((dtype, ) + worst))


# ---- operators and the Python surface ----------------------------------------------------------------------------------
def _pattern():
    """300 x 200, rows 7..11 and columns 50..59 empty, row 123 a hub that holds every other column."""
    rng = np.random.default_rng(12)
    mask = rng.random((300, 200)) < 0.04
    mask[123] = True
    mask[7:12] = False
    mask[:, 50:60] = False
    row, col = np.nonzero(mask)
    return mask, row, col


@pytest.fixture(scope='module')
def pattern():
    return _pattern()


def _adj(ts, dev, pattern, value=None):
    mask, row, col = pattern
    return ts.SparseTensor(row=torch.from_numpy(row).to(dev), col=torch.from_numpy(col).to(dev), value=value,
                           sparse_sizes=mask.shape)


def _dense_attention(mask, row, col, q, k, v, scale, bias=None):
    """Dense masked multi-head attention in the dtype of the operands; rows without entries give zeros."""
    scores = torch.einsum('mhd,nhd->mnh', q, k) * scale
    if bias is not None:
        b = bias if bias.dim() == 2 else bias[:, None].expand(-1, q.size(1))
        scores = scores + torch.zeros_like(scores).index_put((torch.from_numpy(row), torch.from_numpy(col)), b)
    m3 = torch.from_numpy(mask)[:, :, None].expand_as(scores)
    P = torch.softmax(torch.where(m3, scores, torch.full_like(scores, -np.inf)), 1)
    P = torch.where(m3 & ~torch.isnan(P), P, torch.zeros_like(P))
    return torch.einsum('mnh,nhd->mhd', P, v)


def _case_of(A, pattern):
    mask, row, col = pattern
    return F.Case('pattern', tonp(A.storage.rowptr()), col.astype(np.int64), row.size, mask.shape[0], mask.shape[1])


@pytest.mark.parametrize('D', [5, 16])
def test_public_call_against_dense_fp64_and_the_chain(ts, dev, pattern, D):
    mask, row, col = pattern
    H = 3
    rng = np.random.default_rng(140)
    q, k, v = (torch.from_numpy(rng.standard_normal(s)) for s in ((300, H, D), (200, H, D), (200, H, D)))
    b1, b2 = torch.from_numpy(rng.standard_normal(row.size)), torch.from_numpy(rng.standard_normal((row.size, H)))
    for bias in (None, b1, b2):
        A = _adj(ts, dev, pattern, value=None if bias is None else bias.to(dev))
        want = _dense_attention(mask, row, col, q, k, v, 0.3, bias)
        got = A.attention(q.to(dev), k.to(dev), v.to(dev), 0.3, bias=bias is not None)
        assert got.shape == (300, H, D) and got.dtype == torch.float64 and not got.requires_grad
        assert torch.allclose(got.cpu(), want, rtol=1e-11, atol=1e-13) and bool((got[7:12] == 0).all())
        assert bits_equal(got, ts.attention(A, q.to(dev), k.to(dev), v.to(dev), 0.3, bias is not None))
        # float32: the fused call and the chain are both inside the bound, so they differ by at most two bounds
        case = _case_of(A, pattern)
        f = [t.float() for t in (q, k, v)]
        fb = None if bias is None else bias.float()
        A32 = _adj(ts, dev, pattern, value=None if fb is None else fb.to(dev))
        fused = A32.attention(f[0].to(dev), f[1].to(dev), f[2].to(dev), 0.3, bias=fb is not None)
        rowptr, colidx, _ = A32.csr()
        o2, lse = torch.ops.tsamd.attention_heads(rowptr, colidx, None if fb is None else fb.to(dev), f[0].to(dev),
                                                  f[1].to(dev), f[2].to(dev), 0.3)
        assert bits_equal(o2, fused) and lse.shape == (300, H) and lse.dtype == torch.float32
        ex = F.exact(case.ptr, case.ind, None if fb is None else fb.numpy(), f[0].numpy(), f[1].numpy(), f[2].numpy(), 0.3)
        ra = F.check(tonp(fused), tonp(lse), ex, 'f32')
        if bias is None:
            chain = A32.sddmm(f[0].to(dev), f[1].to(dev), 0.3).softmax(1).matmul_heads(f[2].to(dev))
            bo, _ = F.bounds(ex, D, 'f32')
            rb = F._ratio(tonp(chain).astype(np.float64), ex.out, bo, 'chain', 'f32')
            assert bool((np.abs(tonp(chain).astype(np.float64) - tonp(fused)) <= 2 * bo).all())
            print('D = %d float32, worst err / bound: fused out %.3g lse %.3g, chain %.3g' % (D, ra[0], ra[1], rb))


def test_all_gradients_against_fp64_autograd(ts, dev, pattern):
    mask, row, col = pattern
    H = 3
    rng = np.random.default_rng(150)
    for D, form in ((5, 0), (16, 1), (8, 2)):
        q, k, v = (torch.from_numpy(rng.standard_normal(s)) for s in ((300, H, D), (200, H, D), (200, H, D)))
        go = torch.from_numpy(rng.standard_normal((300, H, D)))
        bias = (None, torch.from_numpy(rng.standard_normal(row.size)), torch.from_numpy(rng.standard_normal((row.size, H))))[form]
        leaves = [t.clone().requires_grad_() for t in (q, k, v)] + ([bias.clone().requires_grad_()] if form else [])
        want = torch.autograd.grad(_dense_attention(mask, row, col, *leaves[:3], 0.7, leaves[3] if form else None), leaves, go)
        dl = [t.to(dev).requires_grad_() for t in (q, k, v)] + ([bias.to(dev).requires_grad_()] if form else [])
        A = _adj(ts, dev, pattern, value=dl[3] if form else None)
        assert A.storage._colptr is None and A.storage._csr2csc is None
        out = A.attention(dl[0], dl[1], dl[2], 0.7, bias=bool(form))
        assert out.requires_grad
        got = torch.autograd.grad(out, dl, go.to(dev))
        for g, w, name in zip(got, want, 'qkvb'):
            assert g.shape == w.shape and torch.allclose(g.cpu(), w, rtol=1e-9, atol=1e-12), (D, name)
        # float32 beside the fp64 loops of the reference: sums of up to 200 terms of size one, each carrying a relative
        # error of a few hundred u (the bound of p): 1e-4 absolute
        f = [t.float() for t in (q, k, v)]
        fb = None if not form else bias.float()
        fl = [t.to(dev).requires_grad_() for t in f] + ([fb.to(dev).requires_grad_()] if form else [])
        A32 = _adj(ts, dev, pattern, value=fl[3] if form else None)
        got = torch.autograd.grad(A32.attention(fl[0], fl[1], fl[2], 0.7, bias=bool(form)), fl, go.float().to(dev))
        case = _case_of(A32, pattern)
        gq, gk, gv, ds = F.grads_exact(case.ptr, case.ind, None if fb is None else fb.numpy(), f[0].numpy(), f[1].numpy(),
                                       f[2].numpy(), 0.7, go.float().numpy())
        refs = [gq, gk, gv] + ([ds if form == 2 else ds.sum(1)] if form else [])
        for g, w, name in zip(got, refs, 'qkvb'):
            assert np.allclose(tonp(g), w, rtol=1e-4, atol=1e-4), (D, name, float(np.abs(tonp(g) - w).max()))


def test_gradcheck_on_a_small_pattern(ts, dev):
    rng = np.random.default_rng(160)
    mask = rng.random((12, 9)) < 0.35
    mask[4] = False
    mask[:, 2] = False
    row, col = np.nonzero(mask)
    q, k, v, b1, b2 = (torch.from_numpy(rng.standard_normal(s)).to(dev).requires_grad_()
                       for s in ((12, 2, 3), (9, 2, 3), (9, 2, 3), (row.size, ), (row.size, 2)))
    A = _adj(ts, dev, (mask, row, col))
    assert torch.autograd.gradcheck(lambda a, b, c: A.attention(a, b, c, 0.8), (q, k, v), nondet_tol=0.0)
    for bias in (b1, b2):
        fn = lambda a, b, c, d: A.set_value(d, layout='coo').attention(a, b, c, bias=True)  # noqa: E731
        assert torch.autograd.gradcheck(fn, (q, k, v, bias), nondet_tol=0.0)
    y = A.attention(q, k, v)
    gq, = torch.autograd.grad((y * y).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):  # no second order
        gq.sum().backward()


def test_expanded_and_transposed_grad_out(ts, dev, pattern):
    mask, row, col = pattern
    rng = np.random.default_rng(170)
    H, D = 3, 5
    q, k, v = (torch.from_numpy(rng.standard_normal(s)) for s in ((300, H, D), (200, H, D), (200, H, D)))
    w = torch.from_numpy(rng.standard_normal((300, D, H)))
    A = _adj(ts, dev, pattern)
    for loss in (lambda o, dv: o.sum(), lambda o, dv: (o.transpose(1, 2) * w.to(dv)).sum(),
                 lambda o, dv: (o[:, :, ::2] * 3).sum()):
        g = [t.clone().to(dev).requires_grad_() for t in (q, k, v)]
        loss(A.attention(*g), dev).backward()
        d = [t.clone().requires_grad_() for t in (q, k, v)]
        loss(_dense_attention(mask, row, col, *d, D ** -0.5), 'cpu').backward()
        for a, b in zip(g, d):
            assert torch.allclose(a.grad.cpu(), b.grad, rtol=1e-9, atol=1e-12)


def test_only_the_gradients_asked_for_and_the_column_caches(ts, dev, pattern):
    mask, row, col = pattern
    rng = np.random.default_rng(180)
    H, D = 2, 4
    q, k, v, b = (torch.from_numpy(rng.standard_normal(s)).to(dev) for s in ((300, H, D), (200, H, D), (200, H, D),
                                                                             (row.size, H)))

    def run(which):
        t = {n: a.clone().requires_grad_(n in which) for n, a in (('q', q), ('k', k), ('v', v), ('b', b))}
        A = _adj(ts, dev, pattern, value=t['b'])
        A.attention(t['q'], t['k'], t['v'], bias=True).sum().backward()
        assert [n for n in t if t[n].grad is not None] == list(which)
        return A.storage._colptr is None and A.storage._csr2csc is None

    assert run('q') and run('b') and run('qb'), 'no column-side gradient: the CSC caches stay None'
    assert not run('k') and not run('v') and not run('qkvb')
    A = _adj(ts, dev, pattern)
    with torch.no_grad():
        A.attention(q.clone().requires_grad_(), k.clone().requires_grad_(), v.clone().requires_grad_())
    assert A.storage._colptr is None and A.storage._csr2csc is None


def test_two_dimensional_operands_and_the_default_scale(ts, dev, pattern):
    rng = np.random.default_rng(190)
    D = 6
    q, k, v = (torch.from_numpy(rng.standard_normal(s)).float().to(dev) for s in ((300, D), (200, D), (200, D)))
    A = _adj(ts, dev, pattern)
    flat = A.attention(q, k, v)
    assert flat.shape == (300, D)
    assert bits_equal(flat, A.attention(q[:, None], k[:, None], v[:, None], D ** -0.5)[:, 0])
    assert not bits_equal(flat, A.attention(q, k, v, 1.0))
    g = [t.clone().requires_grad_() for t in (q, k, v)]
    A.attention(*g).sum().backward()
    assert all(t.grad.shape == t.shape for t in g)


def test_scripted_module_calls_the_operators(ts, dev, pattern):
    class Layer(torch.nn.Module):
        def forward(self, rowptr: torch.Tensor, col: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    go: torch.Tensor, scale: float):
            out, lse = torch.ops.tsamd.attention_heads(rowptr, col, None, q, k, v, scale)
            p, ds = torch.ops.tsamd.attention_heads_bw(None, rowptr, col, None, q, k, v, out, lse, go, scale)
            return out, p, ds

    rng = np.random.default_rng(200)
    q, k, v, go = (torch.from_numpy(rng.standard_normal(s)).float().to(dev)
                   for s in ((300, 2, 8), (200, 2, 8), (200, 2, 8), (300, 2, 8)))
    A = _adj(ts, dev, pattern)
    rowptr, col, _ = A.csr()
    got = torch.jit.script(Layer())(rowptr, col, q, k, v, go, 0.35)
    for a, b in zip(got, Layer()(rowptr, col, q, k, v, go, 0.35)):
        assert bits_equal(a, b)
    assert bits_equal(got[0], A.attention(q, k, v, 0.35))
    sums = torch.zeros(300, 2, device=dev).index_add_(0, A.storage.row(), got[1])
    nonempty = (rowptr[1:] > rowptr[:-1])
    assert torch.allclose(sums[nonempty], torch.ones_like(sums[nonempty]), atol=1e-5), 'the probabilities of a row add to 1'


def test_errors(ts, dev, pattern):
    mask, row, col = pattern
    A = _adj(ts, dev, pattern)
    f = lambda *s: torch.ones(*s, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match='heads'):
        A.attention(f(300, 2, 4), f(200, 3, 4), f(200, 3, 4))
    with pytest.raises(ValueError, match='shape of k'):
        A.attention(f(300, 2, 4), f(200, 2, 4), f(200, 2, 8))
    with pytest.raises(ValueError, match='dimensions'):
        A.attention(f(300, 2, 4), f(200, 2, 4), f(200, 8))
    with pytest.raises(ValueError, match='floating'):
        A.attention(f(300, 2, 4).long(), f(200, 2, 4).long(), f(200, 2, 4).long())
    with pytest.raises(ValueError, match='dtype'):
        A.attention(f(300, 2, 4), f(200, 2, 4), f(200, 2, 4).double())
    with pytest.raises(ValueError, match='rows'):
        A.attention(f(299, 2, 4), f(200, 2, 4), f(200, 2, 4))
    with pytest.raises(ValueError, match='columns'):
        A.attention(f(300, 2, 4), f(199, 2, 4), f(199, 2, 4))
    with pytest.raises(ValueError, match='values'):
        A.attention(f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), bias=True)
    with pytest.raises(ValueError, match='bias'):
        A.set_value(f(row.size, 3), layout='coo').attention(f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), bias=True)
    with pytest.raises(ValueError, match='floating'):
        A.set_value(f(row.size).long(), layout='coo').attention(f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), bias=True)
    with pytest.raises(RuntimeError, match='GPU'):
        A.attention(torch.ones(300, 2, 4), torch.ones(200, 2, 4), torch.ones(200, 2, 4))
    rowptr, colidx, _ = A.csr()
    op = torch.ops.tsamd.attention_heads
    with pytest.raises(RuntimeError, match='heads'):
        op(rowptr, colidx, None, f(300, 2, 4), f(200, 3, 4), f(200, 3, 4), 1.0)
    with pytest.raises(RuntimeError, match='shape of k'):
        op(rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 5), 1.0)
    with pytest.raises(RuntimeError, match='entries'):
        op(rowptr, colidx, f(row.size - 1), f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), 1.0)
    with pytest.raises(RuntimeError, match='heads'):
        op(rowptr, colidx, f(row.size, 3), f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), 1.0)
    with pytest.raises(RuntimeError, match='float32, float64, float16 or bfloat16'):
        op(rowptr, colidx, None, f(300, 2, 4).long(), f(200, 2, 4).long(), f(200, 2, 4).long(), 1.0)
    with pytest.raises(RuntimeError, match='dtype'):
        op(rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4).double(), f(200, 2, 4), 1.0)
    with pytest.raises(RuntimeError, match='rowptr'):
        op(rowptr[:-1], colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), 1.0)
    out, lse = op(rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), 1.0)
    with pytest.raises(RuntimeError, match='lse'):
        torch.ops.tsamd.attention_heads_bw(None, rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), out,
                                           lse.double(), f(300, 2, 4), 1.0)
    with pytest.raises(RuntimeError, match='grad_out'):
        torch.ops.tsamd.attention_heads_bw(None, rowptr, colidx, None, f(300, 2, 4), f(200, 2, 4), f(200, 2, 4), out, lse,
                                           f(300, 2, 5), 1.0)
