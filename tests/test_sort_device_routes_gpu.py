"""Which kernels sorted: every device route of csrc/sort.hip, asserted before any value is compared, and the contract
on untrusted ids.

The host decides a plan from the sizes (tests/test_sort_route.py, tests/test_sort_reference.py); whether the bucket
path or the one-sweep passes then sort is decided on the device and left in the workspace header, which the harness of
tests/sort_reference.py reads back from a workspace it owns (tsamd_sort_header).  Every case asserts its host route and
the header's fast word FIRST -- a case that stops reaching its route fails, however exact its values --, then compares
permutation, ids, counts and riding values bit for bit with oracle/np_oracle.py.  Every output and the workspace lie
between guard regions, the workspace starts out full of a sentinel byte, and a second call on the workspace as the
first one left it must give the same bits.

Wild ids (beyond the bit width of their size, or negative) must leave every entry point inside its buffers: fast word
0 -- the bucket kernels never see them --, a permutation, the riding values through it, the unsigned maxima in
counts[2..3].  Ids out of range but inside the width stay on the bucket path and sort exactly as numpy sorts the same
numbers.  (The two-level plans start at 12.5 M entries: tests/test_sort_gpu.py covers them functionally, and no wild id
can reach them either -- one predicate in front of every plan.)"""
import functools

import numpy as np
import pytest
import torch

from oracle import np_oracle as no
from pytorch_sparse_amd import _native as nat
from tests import sort_reference as R

pytestmark = pytest.mark.gpu

CENSUS = {c.name: c for c in R.census()}
VALUES = ('none', 'f32', 'f64')


def _signed(u):
    return int(np.array([u], dtype=np.uint64).view(np.int64)[0])


def _probe_counts(row, col):
    """(#descents, #adjacent duplicates) as the probe counts them: signed lexicographic compare of neighbours;
    (max row, max col) as unsigned numbers."""
    r, c, pr, pc = row[1:], col[1:], row[:-1], col[:-1]
    desc = int(((r < pr) | ((r == pr) & (c < pc))).sum())
    dup = int(((r == pr) & (c == pc)).sum())
    return [desc, dup, _signed(row.astype(np.uint64).max()), _signed(col.astype(np.uint64).max())]


@functools.lru_cache(maxsize=2)
def _expected(name):
    """Input and oracle results of a census case, computed once (host arrays and their device copies)."""
    c = CENSUS[name]
    dev = torch.device('cuda:0')
    row, col = R.make_input(c)
    er, ec, ep = no.sort_coo(row, col, c.M, c.N)
    rng = np.random.default_rng(11)
    val = {'f32': rng.standard_normal(c.E).astype(np.float32), 'i32': rng.integers(-1000, 1000, c.E).astype(np.int32)}
    val['f64'] = val['f32'].astype(np.float64) * 3.0
    key = er * c.N + ec
    head = np.ones(c.E, dtype=bool)
    head[1:] = key[1:] != key[:-1]
    starts = np.nonzero(head)[0]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {
        'row': d(row), 'col': d(col), 'er': d(er), 'ec': d(ec), 'ep': d(ep), 'counts': _probe_counts(row, col),
        'val': {k: d(v) for k, v in val.items()}, 'sval': {k: d(v[ep]) for k, v in val.items()}, 'val_np': val,
        'ep_np': ep, 'row_np': row, 'col_np': col, 'starts': starts, 'k': starts.size,
        'ru': d(er[starts]), 'cu': d(ec[starts]), 'seg': d(np.append(starts, c.E)),
    }


def _assert_host_route(c, vb, coalesce):
    rt = R.route(c.E, c.M, c.N, vb, coalesce)
    assert rt['route'] == 2 and rt['on'] == c.on, ('host route', c.name, rt)
    if c.on:
        assert rt['levels'] == 1 and rt['strip'] == (1 if c.name == 'strip' else 0), ('host route', c.name, rt)
    if c.name == 'posbits':
        assert rt['shift'] == rt['idx_bits'], rt   # the lowest bucket bit is the key's lowest
    return rt


def _assert_route_reached(res, want_fast, what):
    assert res.status == 0, what
    assert res.guards_ok, ('a byte outside an output or the workspace was written', what)
    assert res.hdr['fast'] == want_fast, ('device route: fast word %d, expected %d' % (res.hdr['fast'], want_fast), what)
    assert res.hdr['error'] == 0, what


def _twice(call, check):
    """The call on a fresh (sentinel-filled) workspace, then on that workspace as it was left: the same checks."""
    first = call(None)
    check(first, 'fresh workspace')
    check(call(first.ws), 'dirty workspace')


def _run_values(c):
    x = _expected(c.name)
    for vname in VALUES:
        value = None if vname == 'none' else x['val'][vname]
        _assert_host_route(c, 0 if value is None else value.element_size(), 0)
        for mode in (0, 1, 2, 3):
            want_fast = R.expected_fast(c, mode)
            counts_in = torch.tensor(x['counts'], device=x['row'].device) if mode == 2 else None

            def check(res, ws_state):
                what = (c.name, vname, mode, ws_state)
                _assert_route_reached(res, want_fast, what)
                assert torch.equal(res.out['perm_out'], x['ep']), what
                assert torch.equal(res.out['row_out'], x['er']) and torch.equal(res.out['col_out'], x['ec']), what
                if value is not None:
                    assert torch.equal(res.out['value_out'], x['sval'][vname]), what
                if mode in (1, 3):
                    assert res.out['counts'].tolist()[:2 if mode == 1 else 4] == x['counts'][:2 if mode == 1 else 4], what
                if mode == 1:
                    assert res.hdr['descents'] == x['counts'][0], what

            _twice(lambda ws: R.sort_call('values', x['row'], x['col'], c.M, c.N, mode, counts_in, value, ws=ws), check)


def _run_coalesce(c):
    x = _expected(c.name)
    k = x['k']
    want_fast = R.expected_fast(c, 1)
    for vname in VALUES:
        value = None if vname == 'none' else x['val'][vname]
        _assert_host_route(c, 0 if value is None else value.element_size(), 1)

        def check(res, ws_state):
            what = (c.name, 'coalesce', vname, ws_state)
            _assert_route_reached(res, want_fast, what)
            o = res.out
            assert o['counts'].tolist() == x['counts'][:2] + [k], what
            assert torch.equal(o['row_u'][:k], x['ru']) and torch.equal(o['col_u'][:k], x['cu']), what
            assert torch.equal(o['seg_ptr'][:k + 1], x['seg']), what
            if value is not None:
                assert torch.equal(o['value_out'], x['sval'][vname]), what
            if want_fast:  # the bucket path compacts by itself: the sorted ids are never written
                assert res.untouched['row_tmp'] and res.untouched['col_tmp'], what
            else:
                assert torch.equal(o['row_tmp'], x['er']) and torch.equal(o['col_tmp'], x['ec']), what

        _twice(lambda ws: R.sort_call('coalesce', x['row'], x['col'], c.M, c.N, value=value, ws=ws), check)


def _run_reduce(c):
    x = _expected(c.name)
    k = x['k']
    want_fast = R.expected_fast(c, 1)
    plan = [(vname, code) for vname in ('f32', 'i32') for code in range(4)] + [('none', 0)]
    for vname, code in plan:
        value = None if vname == 'none' else x['val'][vname]
        _assert_host_route(c, 0 if value is None else 4, 1)
        want_fused = 1 if (want_fast and value is not None) else 0
        want_u = None
        if want_fused:
            op = R.REDUCTIONS[code]
            ref = R.reduce_runs(x['val_np'][vname][x['ep_np']], x['starts'], op)
            if vname == 'i32' or op in ('min', 'max'):  # (where numpy's own reduction is exact too: the oracle's)
                assert np.array_equal(ref, no.coalesce(x['row_np'], x['col_np'], x['val_np'][vname], c.M, c.N, op)[2])
            want_u = torch.from_numpy(ref).to(x['row'].device)

        def check(res, ws_state):
            what = (c.name, 'reduce', vname, code, ws_state)
            _assert_route_reached(res, want_fast, what)
            o = res.out
            assert o['counts'].tolist() == x['counts'][:2] + [k, want_fused], ('fused flag against the fast word', what)
            assert torch.equal(o['row_u'][:k], x['ru']) and torch.equal(o['col_u'][:k], x['cu']), what
            if want_fused:   # reduced in the bucket sort: neither the run starts nor the sorted values are written
                assert torch.equal(o['value_u'][:k].view(torch.int32), want_u.view(torch.int32)), what
                assert res.untouched['seg_ptr'] and res.untouched['value_out'], what
            else:
                if value is not None:
                    assert torch.equal(o['value_out'], x['sval'][vname]), what
                if want_fast:   # index only on the bucket path: nobody reduces by the run starts
                    assert res.untouched['seg_ptr'], what
                else:
                    assert torch.equal(o['seg_ptr'][:k + 1], x['seg']), what
            if want_fast:
                assert res.untouched['row_tmp'] and res.untouched['col_tmp'], what
            else:
                assert torch.equal(o['row_tmp'], x['er']) and torch.equal(o['col_tmp'], x['ec']), what

        _twice(lambda ws: R.sort_call('reduce', x['row'], x['col'], c.M, c.N, value=value, reduce=code, ws=ws), check)


RUN = {'values': _run_values, 'coalesce': _run_coalesce, 'reduce': _run_reduce}


@pytest.mark.parametrize('entry', sorted(RUN))
@pytest.mark.parametrize('name', [c.name for c in R.census()])
def test_census_of_device_routes(dev, name, entry):
    RUN[entry](CENSUS[name])


@pytest.mark.parametrize('name', R.RANKED)
def test_census_under_both_rankings(dev, name):
    L = nat.lib()
    try:
        for mode in (0, 1):
            assert L.tsamd_sort_rank_mode(mode) == mode
            for entry in sorted(RUN):
                RUN[entry](CENSUS[name])
    finally:
        L.tsamd_sort_rank_mode(2)


# ---- untrusted ids ----
def _is_permutation(perm, E):
    if perm.numel() != E or bool((perm < 0).any()) or bool((perm >= E).any()):
        return False
    seen = torch.zeros(E, dtype=torch.bool, device=perm.device)
    seen[perm] = True
    return bool(seen.all())


def _wild_entry_points(shape, row_np, col_np, want_fast, what0):
    """Every entry point and mode on ids that may be wild: inside the buffers, the expected route, a permutation with
    the values riding through it, the probe's counts.  The values are the positions themselves (exact in float32 below
    2^24, in float64 always): a sorted value array names the permutation where the entry point returns none."""
    dev = torch.device('cuda:0')
    E = shape.E
    row, col = torch.from_numpy(row_np).to(dev), torch.from_numpy(col_np).to(dev)
    ar = torch.arange(E, device=dev)
    values = {'none': None, 'f32': ar.float(), 'f64': ar.double(), 'i32': ar.int()}
    counts = _probe_counts(row_np, col_np)
    perms = []
    for vname in VALUES:
        value = values[vname]
        for mode in (0, 1, 2, 3):
            what = what0 + ('values', vname, mode)
            cin = torch.tensor([1, 0, 0, 0], device=dev) if mode == 2 else None   # "probed: there are descents"
            res = R.sort_call('values', row, col, shape.M, shape.N, mode, cin, value)
            _assert_route_reached(res, want_fast, what)
            perm = res.out['perm_out']
            assert _is_permutation(perm, E), what
            if value is not None:
                assert torch.equal(res.out['value_out'], value[perm]), what
            if mode in (1, 3):
                assert res.out['counts'].tolist()[:2 if mode == 1 else 4] == counts[:2 if mode == 1 else 4], what
            perms.append(perm.clone())
    assert all(torch.equal(p, perms[0]) for p in perms), what0   # one order, whoever asks
    for entry, vname, code in ([('coalesce', v, 0) for v in VALUES] + [('reduce', 'f32', r) for r in range(4)] +
                               [('reduce', 'i32', 0), ('reduce', 'none', 0)]):
        what = what0 + (entry, vname, code)
        value = values[vname]
        res = R.sort_call(entry, row, col, shape.M, shape.N, value=value, reduce=code)
        _assert_route_reached(res, want_fast, what)
        got = res.out['counts'].tolist()
        assert got[:2] == counts[:2] and 1 <= got[2] <= E, what
        if entry == 'reduce':
            assert got[3] == (1 if want_fast and value is not None else 0), what
        if value is not None and not (entry == 'reduce' and want_fast):
            assert torch.equal(res.out['value_out'].long(), perms[0]), what
    return perms[0]


@pytest.mark.parametrize('where', R.WHERE)
@pytest.mark.parametrize('kind', range(6))
@pytest.mark.parametrize('shape', R.WILD_SHAPES, ids=lambda s: s.name)
def test_wild_ids_never_reach_the_bucket_kernels(dev, shape, kind, where):
    name, which, bad = R.wild_kinds(shape.M, shape.N)[kind]
    for vb in (0, 4, 8):
        for co in (0, 1):
            assert R.route(shape.E, shape.M, shape.N, vb, co)['on'] == 1   # a bucket plan: the path to keep them off
    row, col = R.make_input(shape)
    (row if which == 'row' else col)[R.wild_positions(shape.E, where)] = bad
    assert not R.fits(row, col, R.route(shape.E, shape.M, shape.N)).all()
    _wild_entry_points(shape, row, col, 0, (shape.name, name, where))


@pytest.mark.parametrize('where', ('first', 'percent'))
@pytest.mark.parametrize('kind', range(6))
def test_wild_ids_through_the_passes_of_a_full_word(dev, kind, where):
    """No bucket plan (E = 2^17 - 1), 47 + 17 = 64 bits: the sixth digit reaches past the word, and a wild id sets key
    bits the word cannot hold.  The histogram comes from the word: still a permutation."""
    shape = R.WILD_PASSES_ONLY
    rt = R.route(shape.E, shape.M, shape.N)
    assert rt['on'] == 0 and rt['packed'] == 1 and 8 * rt['passes'] + rt['idx_bits'] > 64
    name, which, bad = R.wild_kinds(shape.M, shape.N)[kind]
    row, col = R.make_input(shape)
    (row if which == 'row' else col)[R.wild_positions(shape.E, where)] = bad
    _wild_entry_points(shape, row, col, 0, (shape.name, name, where))


@pytest.mark.parametrize('where', R.WHERE)
def test_out_of_range_ids_inside_the_bit_width_stay_on_the_bucket_path(dev, where):
    """The control: row = M = 300 (< 2^9) is out of range and not wild -- fast word 1 at every entry point, and the
    order in which numpy sorts the same numbers (row * N + col orders like (row, col) while every col < N).  Then a col
    id in [N, 2^9) as well: the kernels order by (row << 9 | col), restated here."""
    shape = R.WILD_SHAPES[0]
    row, col = R.make_input(shape)
    at = R.wild_positions(shape.E, where)
    row[at] = shape.M
    assert R.fits(row, col, R.route(shape.E, shape.M, shape.N)).all()
    perm = _wild_entry_points(shape, row, col, 1, (shape.name, 'row_M', where))
    er, ec, ep = no.sort_coo(row, col, shape.M, shape.N)
    assert np.array_equal(perm.cpu().numpy(), ep)
    res = R.sort_call('values', torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev), shape.M, shape.N, 3)
    _assert_route_reached(res, 1, 'row_M ids')
    assert np.array_equal(res.out['row_out'].cpu().numpy(), er) and np.array_equal(res.out['col_out'].cpu().numpy(), ec)
    assert res.out['counts'].tolist()[2:] == [shape.M, int(col.max())]
    # a col id in [N, 2^col_bits): the kernels order by (row << 9 | col)
    col[at] = 511
    res = R.sort_call('values', torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev), shape.M, shape.N, 3)
    _assert_route_reached(res, 1, 'col 511')
    ep2 = np.argsort((row << 9) | col, kind='stable')
    assert np.array_equal(res.out['perm_out'].cpu().numpy(), ep2)
    assert np.array_equal(res.out['row_out'].cpu().numpy(), row[ep2]) and np.array_equal(res.out['col_out'].cpu().numpy(), col[ep2])
    assert res.out['counts'].tolist()[2:] == [shape.M, 511]
