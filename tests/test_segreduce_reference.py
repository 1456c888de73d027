"""tests/segreduce_reference.py held to torch's own segment / scatter reductions, its census held to its own
invariants and to the routes the GPU tests rely on, its lane-level restatement of csrc/segreduce.hip accepted by the
comparator and eight planted defects rejected by it; and the status codes tsamd_segment_reduce_balanced returns before
any device call.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import segreduce_reference as R
from tests.util import SUM_ATOL, SUM_TOL, fromnp

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16,
         'i32': torch.int32, 'i64': torch.int64}
CASES = R.cases()
BY_NAME = {c.name: c for c in CASES}


def _tol(dtype):
    return dict(sum_tol=SUM_TOL.get(TORCH[dtype]), sum_atol=SUM_ATOL.get(TORCH[dtype]))


def _torch_reduce(t64, ptr, nseg, reduce):
    """torch.scatter_reduce over the segment ids (include_self=False) -> values on the non-empty segments."""
    lens = np.diff(ptr)
    idx = torch.from_numpy(np.repeat(np.arange(nseg), lens)).view(-1, 1).expand_as(t64)
    red = {'sum': 'sum', 'mean': 'mean', 'min': 'amin', 'max': 'amax'}[reduce]
    return torch.zeros((nseg, t64.shape[1]), dtype=t64.dtype).scatter_reduce(0, idx, t64, red, include_self=False)


def test_case_set_holds_the_layouts_it_names():
    names = [c.name for c in CASES]
    assert names[:9] == ['ruler', 'ones', 'ones_plus_empty', 'empties_leading', 'empties_trailing', 'empties_inside',
                         'one_segment', 'long_aligned', 'long_mid']
    assert [BY_NAME['tail%d' % e].E for e in R.TAIL_SIZES] == list(R.TAIL_SIZES)
    assert all(c.E == int(c.ptr[-1]) and c.nseg == c.ptr.size - 1 and c.E <= 200_000 for c in CASES)
    assert BY_NAME['ones'].nseg == BY_NAME['ones'].E and BY_NAME['one_segment'].nseg == 1
    assert bool((np.diff(BY_NAME['empties_leading'].ptr)[:5000] == 0).all())
    assert bool((np.diff(BY_NAME['empties_trailing'].ptr)[-5000:] == 0).all())
    ruler = BY_NAME['ruler']
    ends = set((ruler.ptr[1:] % R.TILE).tolist())
    assert ends >= {o % R.TILE for o in R.RULER_OFFSETS}
    assert int(BY_NAME['long_aligned'].ptr[1]) > R.CHUNK, 'a fix-up segment that starts at entry 0'
    for name in ('long_aligned', 'long_mid'):
        assert int(np.diff(BY_NAME[name].ptr)[-1]) > 128 * R.CHUNK, 'the last entry closes a 129-chunk run'
    assert R.gate_case(32767).E == 32767 and R.gate_case(32768).E == 32768


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_oracles_against_torch(dtype):
    """reduce_exact and reduce_sequential against torch.scatter_reduce / torch.segment_reduce in fp64 / int64 on the
    non-empty segments (torch leaves its init value in an empty one); empty segments give 0."""
    floating = dtype in R.FLOATS
    for case in (BY_NAME['tail4097'], BY_NAME['empties_inside'], BY_NAME['tail65'], R.gate_case(3000)):
        ne = np.diff(case.ptr) > 0
        for kind in (('integers', 'uniform') if floating else ('integers', )):
            value = R.values(case, kind, dtype, D=2)
            perm = np.random.default_rng(1).permutation(case.E)
            shuffled = np.empty_like(value)
            shuffled[perm] = value
            acc = R.to_acc(value, dtype)
            t64 = torch.from_numpy(acc.astype(np.float64 if floating else np.int64))
            for reduce in R.REDUCES:
                want = _torch_reduce(t64, case.ptr, case.nseg, reduce).numpy()
                exact, l1 = R.reduce_exact(acc, None, case.ptr, case.nseg, reduce)
                assert exact.dtype == (np.float64 if floating else np.int64)
                assert bool((exact[~ne] == 0).all())
                assert (l1 is None) == (not floating or reduce in ('min', 'max'))
                if floating:
                    if reduce in ('min', 'max'):
                        assert np.array_equal(exact[ne], want[ne]), (reduce, kind)
                    else:
                        assert bool((np.abs(exact - want)[ne] <= 1e-13 * l1[ne]).all()), (reduce, kind)
                        sr = torch.segment_reduce(t64, reduce, offsets=torch.from_numpy(case.ptr), axis=0).numpy()
                        assert bool((np.abs(exact - sr)[ne] <= 1e-13 * l1[ne]).all())
                        assert bool((np.abs(exact) <= l1 * (1 + 1e-12)).all())
                else:
                    assert np.array_equal(exact[ne], want[ne]), (reduce, kind)  # integer mean: floor
                ex2, _ = R.reduce_exact(R.to_acc(shuffled, dtype), perm, case.ptr, case.nseg, reduce)
                assert np.array_equal(ex2, exact), 'perm'
                seq = R.reduce_sequential(value, None, case.ptr, case.nseg, reduce, dtype)
                assert R.same_bits(seq, R.reduce_sequential(shuffled, perm, case.ptr, case.nseg, reduce, dtype))
                assert seq.dtype == value.dtype and seq.shape == (case.nseg, 2)
                if kind == 'integers' or reduce in ('min', 'max'):
                    assert R.same_bits(seq, R.store(exact, dtype)), (reduce, kind)
                else:
                    R.check_result(seq, value, None, case.ptr, case.nseg, reduce, dtype, kind, **_tol(dtype))
                # the storage convention is torch's: the same bits as .to(dtype)
                t = fromnp(seq, TORCH[dtype])
                if kind == 'integers' and floating:
                    narrow = dtype in ('f16', 'bf16')  # rounded from the fp32 accumulator
                    assert torch.equal(t, torch.from_numpy(exact).to(torch.float32 if narrow else t.dtype).to(t.dtype))


def test_integer_mean_floors_on_negative_sums():
    ptr = np.array([0, 2, 4, 7], np.int64)
    v = np.array([-3, 0, 3, 0, -7, 0, 0], np.int64)
    for dtype in R.INTS:
        assert R.reduce_exact(v, None, ptr, 3, 'mean')[0].tolist() == [-2, 1, -3]
        assert R.reduce_sequential(R.store(v, dtype), None, ptr, 3, 'mean', dtype).tolist() == [-2, 1, -3]
        assert R.emulate_balanced(R.store(v, dtype), None, ptr, 3, 'mean', dtype).tolist() == [-2, 1, -3]
        assert R.emulate_balanced(R.store(v, dtype), None, ptr, 3, 'mean', dtype,
                                  mutant='mean_truncates').tolist() == [-1, 1, -2]


@pytest.mark.parametrize('dtype', R.FLOATS)
def test_nan_and_tie_rule_of_the_sequential_loop(dtype):
    """acc starts at the first value, a later NaN never replaces it, a NaN result exactly when the first value is NaN,
    ties keep the earlier entry -- on hand-made segments, and the vectorised winners equal to the literal loop on every
    shipped layout."""
    nan = float('nan')
    segs = [[1, nan, 0], [nan, 1, 0], [1, 0, nan], [nan], [nan, nan], [0.0, -0.0], [-0.0, 0.0], [2, -0.0, 0.0, nan],
            [nan, -0.0], [5, nan, nan, 5]]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    flat = np.array([x for s in segs for x in s], np.float64)
    want_min = [0, nan, 0, nan, nan, 0.0, -0.0, -0.0, nan, 5]
    for reduce, values, want in (('min', flat, want_min), ('max', -flat, (-np.array(want_min, np.float64)).tolist())):
        got = R.reduce_sequential(R.store(values, dtype), None, ptr, len(segs), reduce, dtype)
        assert R.same_bits(got, R.store(np.array(want, np.float64), dtype)), (reduce, got)
        assert R.same_bits(got, R.emulate_balanced(R.store(values, dtype), None, ptr, len(segs), reduce, dtype))
    tree = R.emulate_balanced(R.store(flat, dtype), None, ptr, len(segs), 'min', dtype, mutant='nan_tree_rule')
    assert float(R.to_acc(tree, dtype)[0]) == 1.0, 'the scan without the rule: [1, NaN, 0] -> 1'
    if dtype != 'f32':
        return
    for case in CASES:
        for kind in R.KINDS:
            for reduce in ('min', 'max'):
                a = R.to_acc(R.values(case, kind, dtype, reduce, D=1), dtype)
                assert np.array_equal(R._winner(a, case.ptr, reduce)[:, 0], R._winner_loop(a[:, 0], case.ptr, reduce)), \
                    (case.name, kind, reduce)


def test_value_kinds_hold_what_they_claim():
    for case in CASES:
        ne = np.nonzero(np.diff(case.ptr) > 0)[0]
        for reduce in ('min', 'max'):
            z = R.to_acc(R.values(case, 'signed_zero', 'f32', reduce), 'f32')
            ext, _ = R.reduce_exact(z, None, case.ptr, case.nseg, reduce)
            assert bool((ext == 0).all()), 'every extremum is a zero'
            if ne.size >= 16:
                neg = np.signbit(R.reduce_sequential(z, None, case.ptr, case.nseg, reduce, 'f32'))[ne]
                assert neg.any() and not neg.all(), 'both orders of the tie'
                both = np.add.reduceat((z == 0) & np.signbit(z), case.ptr[ne], axis=0)
                pos = np.add.reduceat((z == 0) & ~np.signbit(z), case.ptr[ne], axis=0)
                assert bool(((both > 0) & (pos > 0))[np.diff(case.ptr)[ne] > 1].all()), 'a tie in every segment'
        x = R.to_acc(R.values(case, 'nan', 'f32'), 'f32')
        assert np.isnan(x).any() or case.E < 3
        for dtype in R.FLOATS:
            v = R.to_acc(R.values(case, 'integers', dtype), dtype)
            assert bool((v == np.round(v)).all()) and float(np.abs(v).max()) <= 8
    # the NaN placements the long layouts are there for
    c = BY_NAME['long_mid']
    x = R.to_acc(R.values(c, 'nan', 'f32'), 'f32')
    lens = np.diff(c.ptr)
    j = int(np.argmax(lens))
    s, e = int(c.ptr[j]), int(c.ptr[j + 1])
    win = np.isnan(x[s // 64 * 64 + 64:e // 64 * 64].reshape(-1, 64, 3))
    alone = win.all(axis=1)[1:-1] & ~win.any(axis=1)[:-2] & ~win.any(axis=1)[2:]
    assert alone.any(), 'a window of NaN between two finite windows'
    firsts = np.arange((s // R.CHUNK + 1) * R.CHUNK, e, R.CHUNK)
    assert np.isnan(x[firsts]).any() and not np.isnan(x[firsts]).all(), 'NaN first in a later chunk'
    starts = c.ptr[:-1][lens > 0]
    assert np.isnan(x[starts]).any() and np.isnan(x[c.ptr[1:][lens > 0] - 1]).any()
    allnan = np.add.reduceat(~np.isnan(x), starts, axis=0) == 0
    assert allnan.any(), 'an all-NaN segment'


def test_census_invariants_and_routes():
    cs = R.assert_reaches_every_route(CASES)
    for case, c in zip(CASES, cs):
        ptr, lens = case.ptr, np.diff(case.ptr)
        nch = -(-case.E // R.CHUNK)
        assert c.tile_S.size == -(-case.E // R.TILE) and c.chunk_head.size == nch == c.chunk_tail.size
        assert bool((c.tile_S >= 1).all()) and 0 <= c.idle_waves < R.TILE // R.CHUNK
        # every non-empty segment is written exactly once: by the tile kernel from the chunk that holds it whole, or
        # by the fix-up from the one chunk whose head record names it
        heads = c.chunk_head[c.chunk_head >= 0]
        assert np.array_equal(np.sort(heads), np.nonzero(c.seg_writer == 2)[0]), case.name
        whole = np.nonzero(lens > 0)[0]
        whole = whole[ptr[whole] // R.CHUNK == (ptr[whole + 1] - 1) // R.CHUNK]
        assert np.array_equal(whole, np.nonzero(c.seg_writer == 1)[0]), case.name
        assert int((c.seg_writer > 0).sum()) == int((lens > 0).sum()) == whole.size + heads.size
        assert bool((c.seg_writer[lens == 0] == 0).all())
        # run lengths agree with the segment extents: from the chunk of the first entry to the one before the last
        b = np.nonzero(c.chunk_head >= 0)[0]
        assert np.array_equal(c.chunk_run[b], b - ptr[c.chunk_head[b]] // R.CHUNK), case.name
        assert bool((c.chunk_run[c.chunk_head < 0] == 0).all()) and bool((c.chunk_run[b] >= 1).all())
        # a tail record is the segment that crosses the chunk's end
        t = np.nonzero(c.chunk_tail >= 0)[0]
        ends = np.minimum((t + 1) * R.CHUNK, case.E)
        assert bool((ptr[c.chunk_tail[t]] < ends).all()) and bool((ptr[c.chunk_tail[t] + 1] > ends).all())
    by = dict(zip([c.name for c in CASES], cs))
    assert by['ones'].tile_S[:3].tolist() == [2048] * 3 and bool(by['ones'].tile_staged.all())
    assert by['ones_plus_empty'].tile_S[1] == 2049 and by['ones_plus_empty'].tile_staged.tolist()[:3] == [True, False, True]
    assert by['empties_inside'].tile_staged.tolist() == [True, False, True, True]
    assert sorted(set(by['long_aligned'].chunk_run.tolist())) == [0, 1, 63, 64, 65, 129]
    assert sorted(set(by['long_mid'].chunk_run.tolist())) == [0, 1, 63, 64, 65, 129]
    assert by['long_aligned'].chunk_head[1] == 0, 'the run search of chunk 1 reaches idx < 0'
    with pytest.raises(AssertionError, match='unstaged'):
        R.assert_reaches_every_route([c for c in CASES if c.name not in ('ones_plus_empty', 'empties_inside')])
    with pytest.raises(AssertionError, match='exactly 63'):
        R.assert_reaches_every_route([c for c in CASES if not c.name.startswith('long')])


def _accepts(case, kind, reduce, dtype, mutant=None, D=2):
    value = R.values(case, kind, dtype, reduce, D=D)
    got = R.emulate_balanced(value, None, case.ptr, case.nseg, reduce, dtype, mutant=mutant)
    try:
        R.check_result(got, value, None, case.ptr, case.nseg, reduce, dtype, kind, **_tol(dtype))
    except AssertionError:
        return False
    return True


def _kinds(dtype, reduce):
    if dtype in R.INTS:
        return ('integers', )
    return R.KINDS if reduce in ('min', 'max') else ('integers', 'uniform')


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_comparator_accepts_the_restated_kernel(dtype):
    """The lane-level restatement with the rule in place passes the check the GPU result has to pass: on every layout
    for fp32, on the layouts with long runs, empties and odd tails for the other types."""
    some = ('long_mid', 'empties_inside', 'ones_plus_empty', 'tail513', 'tail4097', 'tail1')
    for case in CASES:
        if dtype != 'f32' and case.name not in some:
            continue
        for reduce in R.REDUCES:
            for kind in _kinds(dtype, reduce):
                assert _accepts(case, kind, reduce, dtype), (case.name, kind, reduce)


# mutant -> (kind, reduce, dtype, layouts that must each expose it, layouts that cannot)
PLANTED = {
    'end_off_by_one': ('integers', 'sum', 'f32', ('tail65', 'ones', 'ruler'), ()),
    'empty_at_init': ('integers', 'min', 'f32', ('empties_inside', 'empties_leading', 'empties_trailing'), ('ones', )),
    'mean_truncates': ('integers', 'mean', 'i64', ('tail4097', 'ruler'), ()),
    'mean_by_chunk_count': ('uniform', 'mean', 'f32', ('long_mid', 'long_aligned', 'ruler'), ('ones', 'tail511')),
    'carry_dropped': ('uniform', 'sum', 'f32', ('one_segment', 'long_aligned', 'long_mid'), ('ones', 'tail63')),
    'fold_at_most_64': ('uniform', 'sum', 'f32', ('long_aligned', 'long_mid'), ('ruler', 'one_segment')),
    'nan_tree_rule': ('nan', 'min', 'f32', ('long_mid', 'ruler', 'tail4097'), ('ones', )),
    'ties_to_later': ('signed_zero', 'max', 'f32', ('long_aligned', 'ruler', 'tail513'), ('ones', )),
}


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_comparator_rejects_planted_defect(mutant):
    kind, reduce, dtype, exposed, blind = PLANTED[mutant]
    for name in exposed:
        assert _accepts(BY_NAME[name], kind, reduce, dtype), 'the unplanted kernel on %s' % name
        assert not _accepts(BY_NAME[name], kind, reduce, dtype, mutant=mutant), '%s not seen on %s' % (mutant, name)
    for name in blind:  # why the layouts above are in the set
        assert _accepts(BY_NAME[name], kind, reduce, dtype, mutant=mutant), name


def test_planted_defects_cover_the_list():
    assert sorted(PLANTED) == sorted(R.MUTANTS) and len(R.MUTANTS) == 8


def test_balanced_entry_status_codes_before_any_device_call():
    """tsamd_segment_reduce_balanced validates in this order, all on the host (so this runs without a GPU)."""
    L = nat.lib()
    i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    fake = vp(0x1000)  # never dereferenced
    fn = L.tsamd_segment_reduce_balanced
    fn.restype = ctypes.c_int

    def call(dtype=0, reduce=0, nseg=3, E=4, D=1, out=fake, ptr=fake):
        return fn(dtype, reduce, fake, None, ptr, i64(nseg), i64(E), i64(D), out, fake, sz(1 << 20), None)

    INVALID, UNSUPPORTED, OK = 1, 2, 0
    assert call(nseg=-1) == INVALID and call(E=-1) == INVALID and call(D=-1) == INVALID
    assert call(reduce=-1) == UNSUPPORTED and call(reduce=4) == UNSUPPORTED
    assert call(dtype=9) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(D=65536) == UNSUPPORTED
    assert call(nseg=0, out=None) == OK and call(D=0, out=None, ptr=None) == OK
    assert call(out=None) == INVALID and call(ptr=None) == INVALID
    # a negative size wins over everything after it, an unknown reduce over an unknown dtype
    assert call(nseg=-1, reduce=9, dtype=42) == INVALID and call(reduce=9, dtype=42, D=70000) == UNSUPPORTED
    ws = L.tsamd_segment_reduce_balanced_workspace_bytes
    ws.restype = ctypes.c_size_t
    assert ws(0, i64(513), i64(1)) == 2 * 256 + 2 * 256  # two chunks: 8 B of fp32 and 16 B of ids, each padded to 256
    assert ws(1, i64(200_000), i64(3)) >= 2 * 8 * 3 * 391 + 2 * 8 * 391
    assert ws(0, i64(0), i64(0)) == ws(0, i64(1), i64(1))
