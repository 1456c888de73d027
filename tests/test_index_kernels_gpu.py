"""The index kernels -- exclusive scan (csrc/scan.hip), ind2ptr / ptr2ind (csrc/convert.hip), select, filter,
scatter_rows and the diag family (csrc/select.hip) -- at every tile, slice, wave and block edge, through the C-ABI,
against the numpy oracles of tests/index_reference.py.  All integer work: every comparison is bit-exact.

Every output and every workspace is a slice of a larger buffer filled with a sentinel byte, with guard elements on both
sides; a workspace slice is EXACTLY as large as its *_workspace_bytes call says.  After a call the guards must be
intact, every element the call must write equals the oracle (which never holds the sentinel: checked), and slots the
call must not write still hold the sentinel.  Every case asserts the census it is named for FIRST (the same assertion
tests/test_index_reference.py makes without a GPU), then compares.

The last part runs the zero-extent and empty-result edges of the SparseTensor methods on top of these kernels against
scipy, with no values, 1-D values and [nnz, 3] values, and holds every cached array of the result to a fresh
computation."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import index_reference as R

pytestmark = pytest.mark.gpu

i64, sz_t = ctypes.c_int64, ctypes.c_size_t
BYTE, GUARD, WS_GUARD = 0x5A, 64, 256
SENT = int(np.frombuffer(bytes([BYTE] * 8), np.int64)[0])


def _sizes():
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_index_route(out) == 0
    return R.sizes_from_route(list(out))


SZ = _sizes()
PRED = {name: code for code, name in enumerate(R.PREDS)}


class Slot:
    """n elements between GUARD sentinel elements on either side, all filled with the sentinel byte"""

    def __init__(self, n, dev, dtype=torch.int64, fill=None):
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=dev)
        self.buf.view(torch.uint8).fill_(BYTE)
        self.t = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.t.view(torch.uint8).fill_(fill)
        self.n = n

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def guards_intact(self):
        b = self.buf.view(torch.uint8)
        es = self.buf.element_size()
        return bool((b[:GUARD * es] == BYTE).all()) and bool((b[(GUARD + self.n) * es:] == BYTE).all())

    def get(self):
        assert self.guards_intact(), 'bytes written outside the output'
        return self.t.cpu().numpy()


class Workspace:
    """exactly `nbytes` bytes, 256-byte aligned, between two guard bands"""

    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes + 2 * WS_GUARD, ), BYTE, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.nbytes = nbytes
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + WS_GUARD)
        self.size = sz_t(nbytes)

    def guards_intact(self):
        return bool((self.buf[:WS_GUARD] == BYTE).all()) and bool((self.buf[WS_GUARD + self.nbytes:] == BYTE).all())


def up(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def ok(status, what):
    nat.check(status, what)
    torch.cuda.synchronize()


def same(got, want, what):
    """bit for bit; the oracle holds no sentinel, so an element that equals it has been written"""
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if want.dtype == np.int64:
        assert not (want == SENT).any()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, '%s: %d of %d elements differ, first at %d: got %d, want %d' % (
        what, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def untouched(got, what):
    assert (got == (SENT if got.dtype == np.int64 else BYTE)).all(), '%s: written where nothing belongs' % what


# ----------------------------------------------------------------------------------------------------------------
# scan
# ----------------------------------------------------------------------------------------------------------------
def run_scan(dev, x, in_place, with_total):
    L, n = nat.lib(), x.size
    ws = Workspace(L.tsamd_exclusive_scan_workspace_bytes(i64(n)), dev)
    src = Slot(n, dev)
    src.t.copy_(torch.from_numpy(x))
    dst = src if in_place else Slot(n, dev)
    total = Slot(1, dev)
    with torch.cuda.device(dev):
        st = L.tsamd_exclusive_scan_i64(src.ptr, dst.ptr, i64(n), total.ptr if with_total else None, ws.ptr, ws.size,
                                        nat.stream_ptr(dev))
    ok(st, 'tsamd_exclusive_scan_i64')
    assert ws.guards_intact(), 'bytes written outside the workspace'
    if not in_place:
        same(src.get(), x, 'the input of an out-of-place scan')
    return dst.get(), total.get()


@pytest.mark.parametrize('case', R.scan_cases(SZ), ids=lambda c: c[0])
def test_scan(dev, case):
    name, n, levels = case
    assert len(R.scan_census(n, SZ)) == levels
    assert nat.lib().tsamd_exclusive_scan_workspace_bytes(i64(n)) == R.scan_workspace_bytes(n, SZ)
    big = R.scan_values(n, 'big', seed=n)
    want, want_total = R.exclusive_scan(big)
    assert n < 2 or (want_total > 1 << 40 and want[1] > 1 << 32)
    for in_place, with_total in itertools.product((False, True), (True, False)):
        got, total = run_scan(dev, big, in_place, with_total)
        same(got, want, 'scan of %d, in place %s' % (n, in_place))
        if with_total:
            same(total, np.array([want_total], np.int64), 'total')
        else:
            untouched(total, 'total')
    for kind in ('first', 'last'):
        x = R.scan_values(n, kind)
        want, want_total = R.exclusive_scan(x)
        got, total = run_scan(dev, x, kind == 'last', True)
        same(got, want, 'scan of %d, %s element only' % (n, kind))
        same(total, np.array([want_total], np.int64), 'total')


# ----------------------------------------------------------------------------------------------------------------
# ind2ptr / ptr2ind
# ----------------------------------------------------------------------------------------------------------------
def run_ind2ptr(dev, ind, M, prefill):
    out = Slot(M + 1, dev, fill=prefill)
    d = up(ind, dev)
    with torch.cuda.device(dev):
        st = nat.lib().tsamd_ind2ptr(p(d), i64(M), i64(ind.size), out.ptr, nat.stream_ptr(dev))
    ok(st, 'tsamd_ind2ptr')
    return out.get()


def run_ptr2ind(dev, ptr):
    M, E = ptr.size - 1, int(ptr[-1])
    out = Slot(E, dev)
    d = up(ptr, dev)
    with torch.cuda.device(dev):
        st = nat.lib().tsamd_ptr2ind(p(d), i64(M), i64(E), out.ptr, nat.stream_ptr(dev))
    ok(st, 'tsamd_ptr2ind')
    return out.get()


@pytest.mark.parametrize('case', R.ind2ptr_cases(SZ), ids=lambda c: c[0])
def test_ind2ptr_and_back(dev, case):
    name, M, ind, want = case
    assert R.ind2ptr_target_ok(R.ind2ptr_census(ind, M, SZ), M, want)
    ptr = R.ind2ptr(ind, M)
    # the result must not depend on what the buffer held: a positive prefill, then the -1 the kernel itself pre-sets
    same(run_ind2ptr(dev, ind, M, BYTE), ptr, 'ind2ptr over a positive prefill')
    same(run_ind2ptr(dev, ind, M, 0xFF), ptr, 'ind2ptr over a prefill of -1')
    same(run_ptr2ind(dev, ptr), ind, 'ptr2ind of the result')


def test_ind2ptr_without_entries(dev):
    for M in (0, 1, SZ.long_run, SZ.long_run + 1):
        same(run_ind2ptr(dev, np.zeros(0, np.int64), M, 0xFF), np.zeros(M + 1, np.int64), 'ind2ptr, E = 0')
        assert run_ptr2ind(dev, np.zeros(M + 1, np.int64)).size == 0


@pytest.mark.parametrize('case', R.ptr2ind_cases(SZ), ids=lambda c: c[0])
def test_ptr2ind(dev, case):
    name, ptr, want = case
    M, E = ptr.size - 1, int(ptr[-1])
    census = R.expand_census(ptr, M, E, SZ)
    assert R.expand_target_ok(census, want), census
    assert ('search' in {r for _, _, _, r in census}) == name.endswith('-search')
    ind = R.ptr2ind(ptr)
    same(run_ptr2ind(dev, ptr), ind, 'ptr2ind')
    same(run_ind2ptr(dev, ind, M, BYTE), ptr, 'ind2ptr of the result')


# ----------------------------------------------------------------------------------------------------------------
# select
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def source(dev):
    ptr, S, ind, _ = R.select_source(SZ)
    return dict(ptr=ptr, S=S, ind=ind, d_ptr=up(ptr, dev), d_ind=up(ind, dev))


def run_select_plan(dev, src, idx):
    L, K = nat.lib(), idx.size
    ws = Workspace(L.tsamd_select_workspace_bytes(i64(K)), dev)
    out_ptr, info = Slot(K + 1, dev), Slot(2, dev)
    d_idx = up(idx, dev)
    with torch.cuda.device(dev):
        st = L.tsamd_select_plan(p(src['d_ptr']), i64(src['S']), p(d_idx), i64(K), out_ptr.ptr, info.ptr, ws.ptr, ws.size,
                                 nat.stream_ptr(dev))
    ok(st, 'tsamd_select_plan')
    assert ws.guards_intact(), 'bytes written outside the workspace'
    return out_ptr.get(), info.get(), d_idx


def run_select_fill(dev, src, d_idx, K, out_ptr, total, outs=(True, True, True)):
    slots = [Slot(total, dev) if on else None for on in outs]
    d_out_ptr = up(out_ptr, dev)
    with torch.cuda.device(dev):
        st = nat.lib().tsamd_select_fill(p(src['d_ptr']), i64(src['S']), p(src['d_ind']), p(d_idx), i64(K), p(d_out_ptr),
                                         i64(total), *[s.ptr if s else None for s in slots], nat.stream_ptr(dev))
    ok(st, 'tsamd_select_fill')
    return [s.get() if s else None for s in slots]


@pytest.mark.parametrize('case', R.select_cases(SZ), ids=lambda c: c[0])
def test_select(dev, source, case):
    name, idx, want = case
    ptr, S, ind = source['ptr'], source['S'], source['ind']
    plan = R.select_plan(ptr, S, idx)
    census = R.expand_census(plan[0], idx.size, plan[1], SZ)
    assert R.select_target_ok(census, plan, want), (census, plan[1:])
    assert ('search' in {r for _, _, _, r in census}) == name.endswith('-search')
    out_ptr, info, d_idx = run_select_plan(dev, source, idx)
    same(out_ptr, plan[0], 'out_ptr')
    same(info, np.array([plan[1], plan[2]], np.int64), 'info = (total, ids out of range)')
    oracle = R.select_fill(ptr, S, ind, idx)
    # all eight NULL / non-NULL combinations where a tile edge or the search route is involved, all three otherwise
    edge = 'tile' in name or 'search' in name or 'invalid' in name
    for outs in itertools.product((True, False), repeat=3) if edge else [(True, True, True)]:
        got = run_select_fill(dev, source, d_idx, idx.size, plan[0], plan[1], outs)
        for g, w, what in zip(got, oracle, ('seg_out', 'ind_out', 'pos_out')):
            if g is not None:
                same(g, w, '%s with outputs %s' % (what, outs))


# ----------------------------------------------------------------------------------------------------------------
# filter
# ----------------------------------------------------------------------------------------------------------------
def filter_args(dev, pred, inp):
    d = {k: up(inp[k], dev) for k in ('row', 'col', 'mask', 'map')}
    n = inp['row'].size
    return d, (PRED[pred], p(d['row']), p(d['col']), p(d['mask']), p(d['map']), i64(n), i64(inp['a']), i64(inp['b']))


def run_filter(dev, pred, inp, route, maps=(None, None), shifts=(0, 0), outs=(True, True, True)):
    """route 'plan-apply' | 'count-write' -> (count, [row_out, col_out, src_out], pos or None).  The outputs have one
    slot per INPUT entry: the slots past the count must stay untouched."""
    L, n = nat.lib(), inp['row'].size
    keep_alive, head = filter_args(dev, pred, inp)
    d_maps = [up(m, dev) for m in maps]
    count = Slot(1, dev)
    slots = [Slot(n, dev) if on else None for on in outs]
    tail = (p(d_maps[0]), p(d_maps[1]), i64(shifts[0]), i64(shifts[1]), *[s.ptr if s else None for s in slots],
            nat.stream_ptr(dev))
    pos = None
    with torch.cuda.device(dev):
        if route == 'plan-apply':
            ws = Workspace(L.tsamd_filter_workspace_bytes(i64(n)), dev)
            pos_slot = Slot(n + 1, dev)
            ok(L.tsamd_filter_plan(*head, pos_slot.ptr, count.ptr, ws.ptr, ws.size, nat.stream_ptr(dev)), 'tsamd_filter_plan')
            pos = pos_slot.get()
            ok(L.tsamd_filter_apply(pos_slot.ptr, head[1], head[2], head[5], *tail), 'tsamd_filter_apply')
            same(pos_slot.get(), pos, 'pos after the apply')
        else:
            ws = Workspace(L.tsamd_filter_tiles_workspace_bytes(i64(n)), dev)
            ok(L.tsamd_filter_count(*head, count.ptr, ws.ptr, ws.size, nat.stream_ptr(dev)), 'tsamd_filter_count')
            ok(L.tsamd_filter_write(*head, ws.ptr, *tail), 'tsamd_filter_write')
    assert ws.guards_intact(), 'bytes written outside the workspace'
    return int(count.get()[0]), [s.get() if s else None for s in slots], pos


def check_filter(dev, pred, inp, keep, **kw):
    maps, shifts = kw.get('maps', (None, None)), kw.get('shifts', (0, 0))
    want_pos, want_count = R.filter_positions(keep)
    want = R.filter_compact(keep, inp['row'], inp['col'], maps[0], maps[1], shifts[0], shifts[1])
    for route in ('plan-apply', 'count-write'):
        count, got, pos = run_filter(dev, pred, inp, route, **kw)
        assert count == want_count, (route, count, want_count)
        if pos is not None:
            same(pos, want_pos, 'pos')
        for g, w, what in zip(got, want, ('row_out', 'col_out', 'src_out')):
            if g is not None:
                same(g[:count], w, '%s by %s' % (what, route))
                untouched(g[count:], '%s past the count by %s' % (what, route))


@pytest.mark.parametrize('pred', R.PREDS)
def test_filter_plan_apply_and_count_write(dev, pred):
    """both routes x this predicate, every size and keep pattern of the list"""
    for name, n, pattern, variant in R.filter_cases(SZ):
        keep = R.keep_pattern(pattern, n, SZ)
        assert R.filter_target_ok(pattern, n, R.filter_census(keep, SZ), SZ), name
        inp = R.filter_inputs(pred, keep, variant)
        check_filter(dev, pred, inp, keep)


@pytest.mark.parametrize('pred', R.PREDS)
def test_filter_maps_shifts_and_null_outputs(dev, pred):
    s, T = SZ.filter_slice, SZ.filter_tile
    rng = np.random.default_rng(77)
    for n in (s + 1, T + 1, 3 * T + 300):
        keep = R.keep_pattern('random-50pct', n, SZ, seed=3)
        inp = R.filter_inputs(pred, keep, n)
        row_map = rng.integers(0, 1 << 40, inp['M']).astype(np.int64)
        col_map = inp['map'] if pred == 'col_mapped' else rng.integers(0, 1 << 40, inp['N']).astype(np.int64)
        for maps, shifts in (((row_map, col_map), (0, 0)), ((row_map, None), (5, -7)), ((None, col_map), (-1, 1 << 33)),
                             ((None, None), (11, 13))):
            check_filter(dev, pred, inp, keep, maps=maps, shifts=shifts)
        for outs in itertools.product((True, False), repeat=3):
            check_filter(dev, pred, inp, keep, maps=(row_map, col_map), shifts=(2, 3), outs=outs)


def test_filter_mask_rank_map(dev):
    """TSAMD_KEEP_MASK with row = col = NULL: pos is the rank of every set byte (the new id of a kept row / column)"""
    for n in (1, SZ.filter_slice + 1, SZ.scan_tile, SZ.scan_tile + 1):
        keep = R.keep_pattern('random-50pct', n, SZ)
        inp = dict(row=np.zeros(n, np.int64), col=None, mask=np.where(keep, 255, 0).astype(np.uint8), map=None, a=0, b=0)
        L = nat.lib()
        ws, pos, count = Workspace(L.tsamd_filter_workspace_bytes(i64(n)), dev), Slot(n + 1, dev), Slot(1, dev)
        d = up(inp['mask'], dev)
        with torch.cuda.device(dev):
            ok(L.tsamd_filter_plan(PRED['mask'], None, None, p(d), None, i64(n), i64(0), i64(0), pos.ptr, count.ptr, ws.ptr,
                                   ws.size, nat.stream_ptr(dev)), 'tsamd_filter_plan')
        want_pos, want_count = R.filter_positions(keep)
        same(pos.get(), want_pos, 'rank map')
        assert int(count.get()[0]) == want_count and ws.guards_intact()


# ----------------------------------------------------------------------------------------------------------------
# scatter_rows
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.scatter_cases(SZ), ids=lambda c: c[0])
def test_scatter_rows(dev, case):
    name, M, ops = case
    _, deltas = R.cat_plan([r for r, _, _ in ops], M)
    want = R.cat_columns(ops, M)
    total = want[0].size
    assert sorted(want[2].tolist()) == list(range(total))
    combos = itertools.product((True, False), repeat=3) if name.startswith('three') else [(True, True, True)]
    for outs in combos:
        slots = [Slot(total, dev) if on else None for on in outs]
        shift = offset = 0
        for (row, col, width), delta in zip(ops, deltas):
            d = [up(x, dev) for x in (row, col, delta)]
            with torch.cuda.device(dev):
                st = nat.lib().tsamd_scatter_rows(p(d[0]), p(d[1]), i64(row.size), p(d[2]), i64(shift), i64(offset),
                                                  *[s.ptr if s else None for s in slots], nat.stream_ptr(dev))
            ok(st, 'tsamd_scatter_rows')
            shift, offset = shift + width, offset + row.size
        # the operands' slots cover the output exactly once: every element written, src_out a permutation
        for s, w, what in zip(slots, want, ('row_out', 'col_out', 'src_out')):
            if s is not None:
                same(s.get(), w, '%s with outputs %s' % (what, outs))


# ----------------------------------------------------------------------------------------------------------------
# diag
# ----------------------------------------------------------------------------------------------------------------
def run_diag(dev, M, N, k, row, col):
    """-> dict(num_diag, mask, insert or None, set): every device result of the diag family for one pattern"""
    L, E = nat.lib(), row.size
    nd = int(L.tsamd_num_diag(i64(M), i64(N), i64(k)))
    assert nd == R.num_diag(M, N, k)
    d_row, d_col = up(row, dev), up(col, dev)
    dims = (i64(E), i64(M), i64(N), i64(k))
    res = {'num_diag': nd}
    with torch.cuda.device(dev):
        stream = nat.stream_ptr(dev)
        mask = Slot(E + nd, dev, dtype=torch.uint8)
        ok(L.tsamd_non_diag_mask(p(d_row), p(d_col), *dims, mask.ptr, stream), 'tsamd_non_diag_mask')
        res['mask'] = mask.get()
        if not (col - row == k).any():
            outs = [Slot(E + nd, dev) for _ in range(3)]
            ok(L.tsamd_insert_diag(p(d_row), p(d_col), *dims, *[s.ptr for s in outs], stream), 'tsamd_insert_diag')
            res['insert'] = [s.get() for s in outs]
        ws, pos, count = Workspace(L.tsamd_filter_workspace_bytes(i64(E)), dev), Slot(E + 1, dev), Slot(1, dev)
        ok(L.tsamd_filter_plan(PRED['off_diag'], p(d_row), p(d_col), None, None, i64(E), i64(k), i64(0), pos.ptr, count.ptr,
                               ws.ptr, ws.size, stream), 'tsamd_filter_plan')
        assert ws.guards_intact()
        kept = int(count.get()[0])
        outs = [Slot(kept + nd, dev) for _ in range(3)]
        ok(L.tsamd_set_diag_apply(pos.ptr, p(d_row), p(d_col), *dims, *[s.ptr for s in outs], stream), 'tsamd_set_diag_apply')
        res['set'] = (pos.get(), kept, [s.get() for s in outs])
    return res


def check_diag(dev, case):
    name, M, N, k, kind, row, col = case
    res = run_diag(dev, M, N, k, row, col)
    same(res['mask'], R.non_diag_mask(row, col, M, N, k), name + ': non_diag_mask')
    if 'insert' in res:
        for g, w, what in zip(res['insert'], R.insert_diag(row, col, M, N, k), ('row', 'col', 'src')):
            same(g, w, '%s: insert_diag %s' % (name, what))
    else:
        assert kind != 'none'
    pos, count, r, c, s = R.set_diag(row, col, M, N, k)
    same(res['set'][0], pos, name + ': pos')
    assert res['set'][1] == count
    for g, w, what in zip(res['set'][2], (r, c, s), ('row', 'col', 'src')):
        same(g, w, '%s: set_diag %s' % (name, what))


@pytest.mark.parametrize('shape', ('3x6', '4x4', '6x2', '5x5', '5x6'))
def test_diag_small_move_and_fill(dev, shape):
    """every k from -(M + 1) to N + 1, patterns with the whole diagonal, part of it, none of it, and E = 0"""
    cases = [c for c in R.diag_small_cases() if c[0].startswith(shape + '-')]
    assert len(cases) >= 6
    seen = set()
    for case in cases:
        census = R.diag_census(case[5].size, *case[1:4])
        seen.add((census['move'] > 0, census['fill'] > 0))
        check_diag(dev, case)
    assert (True, True) in seen


@pytest.mark.parametrize('case', R.diag_large_cases(), ids=lambda c: c[0])
def test_diag_large_move_and_fill_over_blocks(dev, case):
    _, M, N, k, kind, row, col = case
    census = R.diag_census(row.size, M, N, k)
    assert census['move'] > 1 and census['fill'] == (3 if abs(k) <= 200 else 1)
    check_diag(dev, case)


# ----------------------------------------------------------------------------------------------------------------
# zero-extent and empty results through SparseTensor, against scipy
# ----------------------------------------------------------------------------------------------------------------
MODES = ('no-value', 'value-1d', 'value-2d')


@pytest.fixture(scope='module')
def ts():
    import pytorch_sparse_amd
    return pytorch_sparse_amd


def make(ts, dev, M, N, nnz, seed, mode):
    """-> (SparseTensor, scipy CSR whose data are 1 + the position of the entry, values as numpy or None)"""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    key = np.sort(rng.choice(M * N, nnz, replace=False)) if nnz else np.zeros(0, np.int64)
    row, col = (key // N).astype(np.int64), (key % N).astype(np.int64)
    value = None
    if mode != 'no-value':
        value = rng.integers(1, 100, (nnz, ) if mode == 'value-1d' else (nnz, 3)).astype(np.float32)
    A = ts.SparseTensor(row=up(row, dev), col=up(col, dev), value=up(value, dev), sparse_sizes=(M, N), is_sorted=True)
    S = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.float64), (row, col)), shape=(M, N))
    return A, S, value


def agrees(ts, out, S, value, fill=None):
    """pattern and sizes as scipy's; values gathered by the positions scipy's data carry (-1: a filled entry); every
    cached array of the result as a fresh computation"""
    S = S.tocsr()
    S.sort_indices()
    assert tuple(out.sparse_sizes()) == S.shape
    rowptr, col, val = out.csr()
    np.testing.assert_array_equal(rowptr.cpu().numpy(), S.indptr.astype(np.int64))
    np.testing.assert_array_equal(col.cpu().numpy(), S.indices.astype(np.int64))
    row = out.storage.row()
    np.testing.assert_array_equal(row.cpu().numpy(), S.tocoo().row.astype(np.int64))
    assert rowptr.dtype == col.dtype == row.dtype == torch.int64
    if value is None:
        assert val is None
    else:
        src = S.data.astype(np.int64)
        want = value[np.maximum(src, 1) - 1] if value.shape[0] else np.zeros((src.size, ) + value.shape[1:], np.float32)
        if fill is not None:
            want = np.where((src < 0).reshape((-1, ) + (1, ) * (value.ndim - 1)), np.float32(fill), want)
        assert tuple(val.shape) == want.shape
        np.testing.assert_array_equal(val.cpu().numpy(), want)
    st = out.storage
    fresh = ts.SparseTensor(row=row, col=col, sparse_sizes=out.sparse_sizes(), is_sorted=True).storage
    for key in st.cached_keys():
        np.testing.assert_array_equal(getattr(st, key)().cpu().numpy(), getattr(fresh, key)().cpu().numpy(), err_msg=key)
    for key in ('rowcount', 'colptr', 'colcount', 'csr2csc', 'csc2csr'):  # and what the result computes on demand
        np.testing.assert_array_equal(getattr(st, key)().cpu().numpy(), getattr(fresh, key)().cpu().numpy(), err_msg=key)


@pytest.mark.parametrize('mode', MODES)
def test_empty_selections(ts, dev, mode):
    import scipy.sparse as sp
    A, S, value = make(ts, dev, 23, 31, 300, 1, mode)
    A.storage.colptr(), A.storage.csr2csc(), A.storage.rowcount(), A.storage.colcount()  # caches to hand over
    none = torch.zeros(0, dtype=torch.long, device=dev)
    agrees(ts, A.index_select(0, none), S[[], :], value)
    agrees(ts, A.index_select(1, none), S[:, []], value)
    for start in (0, 7, 31):
        agrees(ts, A.narrow(1, start, 0), S[:, start:start], value)
    for start in (0, 7, 23):
        agrees(ts, A.narrow(0, start, 0), S[start:start, :], value)
    for dim, n in ((0, 23), (1, 31)):
        off, on = torch.zeros(n, dtype=torch.bool, device=dev), torch.ones(n, dtype=torch.bool, device=dev)
        agrees(ts, A.masked_select(dim, off), S[[], :] if dim == 0 else S[:, []], value)
        agrees(ts, A.masked_select(dim, on), S, value)
    agrees(ts, A.masked_select_nnz(torch.zeros(300, dtype=torch.bool, device=dev)), sp.csr_matrix((23, 31)), value)
    agrees(ts, A.masked_select_nnz(torch.ones(300, dtype=torch.bool, device=dev)), S, value)


def with_diag(S, k, marker=-1.0):
    """scipy: the entries off the k-th diagonal + the whole diagonal with `marker` as data"""
    import scipy.sparse as sp
    C = S.tocoo()
    off = C.col - C.row != k
    M, N = S.shape
    d = np.arange(M)
    d = d[(d + k >= 0) & (d + k < N)]
    return sp.csr_matrix((np.concatenate((C.data[off], np.full(d.size, marker))),
                          (np.concatenate((C.row[off], d)), np.concatenate((C.col[off], d + k)))), shape=S.shape)


def without_diag(S, k):
    import scipy.sparse as sp
    C = S.tocoo()
    off = C.col - C.row != k
    return sp.csr_matrix((C.data[off], (C.row[off], C.col[off])), shape=S.shape)


@pytest.mark.parametrize('mode', MODES)
def test_diag_edges(ts, dev, mode):
    for M, N, nnz in ((9, 14, 0), (14, 9, 0), (6, 6, 0), (9, 14, 40), (14, 9, 40)):
        A, S, value = make(ts, dev, M, N, nnz, 2, mode)
        for k in (0, 1, -1, N - 1, N, N + 3, -(M - 1), -M, -(M + 3)):
            agrees(ts, A.fill_diag(7.0, k), with_diag(S, k), value, fill=7.0)
            agrees(ts, A.remove_diag(k), without_diag(S, k), value)
        want = np.zeros((min(M, N), ) + (() if value is None else value.shape[1:]), np.float32)
        C = S.tocoo()
        on = C.row == C.col
        want[C.row[on]] = 1.0 if value is None else value[C.data[on].astype(np.int64) - 1]
        got = A.get_diag()
        assert tuple(got.shape) == want.shape
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('mode', MODES)
def test_cat_with_an_empty_operand(ts, dev, mode):
    import scipy.sparse as sp
    A, SA, va = make(ts, dev, 12, 9, 60, 3, mode)
    B, SB, vb = make(ts, dev, 12, 9, 0, 4, mode)
    C, SC, vc = make(ts, dev, 12, 9, 45, 5, mode)
    for ops in ((A, SA, va), (B, SB, vb), (C, SC, vc)), ((B, SB, vb), (A, SA, va)), ((A, SA, va), (B, SB, vb)), \
            ((B, SB, vb), (B, SB, vb)):
        value = None if va is None else np.concatenate([v for _, _, v in ops])
        offs = np.cumsum([0] + [s.nnz for _, s, _ in ops])
        mats = []
        for (_, s, _), o in zip(ops, offs):
            s = s.copy()
            s.data = s.data + o  # positions count through the operands, as the concatenated values do
            mats.append(s)
        agrees(ts, ts.cat([t for t, _, _ in ops], dim=0), sp.vstack(mats), value)
        agrees(ts, ts.cat([t for t, _, _ in ops], dim=1), sp.hstack(mats), value)
