"""tests/softmax_reference.py held to torch.softmax and torch.autograd in float64, its bounds shown attainable by
torch's own float32 / bfloat16 softmax, its census held to the routes the GPU tests rely on, eight planted defects
rejected by its comparators; and the answers of the softmax entry points that need no device.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import softmax_reference as R
from tests.util import fromnp, tonp

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
CASES = R.cases()
BY_NAME = {c.name: c for c in CASES}


def _per_segment(fn, t, ptr):
    """fn (a softmax over dim 1 of [count, len, D]) applied to every segment of t [E, D]; segments of one length are
    stacked, so the Python loop runs over the distinct lengths only."""
    out = torch.zeros_like(t)
    lens = np.diff(ptr)
    for n in np.unique(lens[lens > 0]):
        idx = (ptr[:-1][lens == n][:, None] + np.arange(n)[None, :]).reshape(-1)
        out[idx] = fn(t[idx].view(-1, int(n), t.shape[1])).reshape(-1, t.shape[1])
    return out


def _softmax(x):
    """torch.softmax over dim 1 of [count, len, D], every (segment, head) contiguous (torch's kernel for the last
    dimension; its strided one adds 34 000 terms one after the other)."""
    return torch.softmax(x.transpose(1, 2).contiguous(), 2).transpose(1, 2)


def _torch_softmax(value_np, perm, case, dtype, compute):
    """torch.softmax per segment in `compute`, rounded to `dtype`; stored elements in the input's own order."""
    t = fromnp(value_np, TORCH[dtype]).to(compute)
    p = np.arange(case.E) if perm is None else perm
    ys = _per_segment(_softmax, t[p], case.ptr)
    y = torch.zeros_like(ys)
    y[p] = ys
    return tonp(y.to(TORCH[dtype]))


def test_route_constants_and_layouts():
    assert (R.CHUNK, R.TILE, R.STAGED, R.FOLD) == R.route()
    assert R.TILE % R.CHUNK == 0 and R.CHUNK % 64 == 0 and R.FOLD >= 1
    assert [c.name for c in CASES] == ['no_segments', 'no_entries', 'single', 'lengths', 'boundaries', 'hub',
                                       'unstaged', 'empties']
    assert all(c.E == int(c.ptr[-1]) and c.nseg == c.ptr.size - 1 and c.E < 100_000 for c in CASES)
    assert (BY_NAME['no_segments'].nseg, BY_NAME['no_entries'].E, BY_NAME['no_entries'].nseg) == (0, 0, 5)
    cs = dict(zip(BY_NAME, R.assert_reaches_every_route(CASES)))
    assert int(np.diff(BY_NAME['hub'].ptr).max()) == (R.FOLD + 2) * R.CHUNK + 1
    assert int(cs['hub'].seg_records.max()) > R.FOLD, 'more records than one fold round holds'
    assert not bool(cs['unstaged'].tile_staged[0]) and bool(cs['lengths'].tile_staged.all())
    b = BY_NAME['boundaries']
    cut = cs['boundaries'].seg_route == 2
    assert bool(((b.ptr[1:] % R.CHUNK == 0) & cut).any()), 'a cut segment that ends on a chunk boundary'
    assert bool(((b.ptr[:-1] % R.CHUNK == 0) & cut).any()), 'a cut segment that starts on one'
    lens = np.diff(BY_NAME['empties'].ptr)
    assert lens[0] == 0 and lens[-1] == 0 and bool((lens[1:-1] == 0).any())
    with pytest.raises(AssertionError):
        R.assert_reaches_every_route([c for c in CASES if c.name != 'hub'])
    with pytest.raises(AssertionError, match='staging'):
        R.assert_reaches_every_route([c for c in CASES if c.name != 'unstaged'])


def test_value_kinds_hold_what_they_claim():
    hub = BY_NAME['hub']
    j = int(np.argmax(np.diff(hub.ptr)))
    s, e = int(hub.ptr[j]), int(hub.ptr[j + 1])
    x = R.values(hub, 'late_max', 'f32')
    assert bool((x[s:e].argmax(axis=0) == e - s - 1).all())
    assert float(R.values(hub, 'big', 'f32').min()) > 88.8, 'exp overflows fp32 without the max subtraction'
    x = R.values(hub, 'neg_inf_piece', 'f32')
    b = (s // R.CHUNK + 1) * R.CHUNK
    assert np.isneginf(x[s:b]).all() and np.isneginf(x[b + R.CHUNK:b + 2 * R.CHUNK]).all()
    assert np.isfinite(x[b:b + R.CHUNK]).any() and np.isfinite(x[b + 2 * R.CHUNK:e]).any()
    assert np.isneginf(R.values(hub, 'all_neg_inf', 'f32')[s:e]).all()
    x = R.values(hub, 'nan_one_head', 'f32')
    assert int(np.isnan(x).sum()) == 1 and bool(np.isnan(x[s:e, 1]).any())
    assert bool(np.isposinf(R.values(hub, 'pos_inf', 'f32')[s:e]).any())


@pytest.mark.parametrize('kind', R.KINDS)
def test_oracle_is_torch_softmax_and_autograd_in_float64(kind):
    """forward_exact == torch.softmax per segment in float64 (non-finite positions included), through a perm as well;
    backward_exact == torch.autograd of that softmax."""
    for case in CASES:
        if case.E == 0:
            y, _, _ = R.forward_exact(np.zeros((0, 3)), None, case.ptr, case.nseg)
            assert y.shape == (0, 3)
            continue
        v = R.values(case, kind, 'f64')
        perm = np.random.default_rng(2).permutation(case.E)
        for p in (None, perm):
            y, dist, n = R.forward_exact(v, p, case.ptr, case.nseg)
            want = _torch_softmax(v, p, case, 'f64', torch.float64)
            assert np.array_equal(np.isnan(y), np.isnan(want)) and np.array_equal(y == 0, want == 0), case.name
            ok = ~np.isnan(y)
            assert bool((np.abs(y - want)[ok] <= 1e-12 * want[ok]).all()), case.name
        if kind not in ('normal', 'late_max', 'big'):
            continue
        t = torch.from_numpy(v).requires_grad_()
        g = torch.from_numpy(R.grads(case, 'f64'))
        ys = _per_segment(_softmax, t, case.ptr)
        ys.backward(g)
        gv, mass, _ = R.backward_exact(ys.detach().numpy(), g.numpy(), None, case.ptr, case.nseg)
        assert bool((np.abs(gv - t.grad.numpy()) <= 1e-12 * mass + 1e-300).all()), case.name


@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
def test_bounds_are_attainable_by_torch_in_float32(dtype):
    """torch.softmax per segment in float32 (rounded once for the 16-bit types) passes the forward comparator on every
    layout and kind, and the float32 expression y * (g - sum g y) the backward one: the reference alone stays within the
    bounds."""
    worst_f = worst_b = 0.0
    for case in CASES:
        if case.E == 0:
            continue
        perm = np.random.default_rng(3).permutation(case.E)
        for kind in R.KINDS:
            v = R.values(case, kind, dtype)
            for p in (None, perm):
                got = _torch_softmax(v, p, case, dtype, torch.float32)
                worst_f = max(worst_f, R.check_forward(got, v, p, case.ptr, case.nseg, dtype))
        y = _torch_softmax(R.values(case, 'normal', dtype), None, case, dtype, torch.float32)
        g = R.grads(case, dtype)
        yt, gt = fromnp(y, TORCH[dtype]).float(), fromnp(g, TORCH[dtype]).float()
        seg = torch.from_numpy(np.repeat(np.arange(case.nseg), np.diff(case.ptr)))
        dot = torch.zeros(case.nseg, 3).index_add_(0, seg, gt * yt)
        gv = tonp((yt * (gt - dot[seg])).to(TORCH[dtype]))
        worst_b = max(worst_b, R.check_backward(gv, y, g, None, case.ptr, case.nseg, dtype))
    print('%s: worst err / bound forward %.3g backward %.3g' % (dtype, worst_f, worst_b))
    assert worst_f <= 1.0 and worst_b <= 1.0


def _accepts(case, kind, dtype, mutant, perm=None):
    v = R.values(case, 'normal' if kind == 'backward' else kind, dtype)
    if perm is not None:
        shuffled = np.empty_like(v)
        shuffled[perm] = v
        v = shuffled
    try:
        if mutant == 'bw_no_dot' or kind == 'backward':
            y = R.emulate_forward(R.values(case, 'normal', dtype), None, case.ptr, case.nseg, dtype)
            g = R.grads(case, dtype)
            got = R.emulate_backward(y, g, None, case.ptr, case.nseg, dtype, mutant=mutant)
            R.check_backward(got, y, g, None, case.ptr, case.nseg, dtype)
        else:
            got = R.emulate_forward(v, perm, case.ptr, case.nseg, dtype, mutant=mutant)
            R.check_forward(got, v, perm, case.ptr, case.nseg, dtype)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize('dtype', R.FLOATS)
def test_comparators_accept_the_softmax_by_pieces(dtype):
    for case in CASES:
        if case.E == 0:
            continue
        for kind in R.KINDS + ('backward', ):
            assert _accepts(case, kind, dtype, None), (case.name, kind)
        assert _accepts(case, 'normal', dtype, None, perm=np.random.default_rng(4).permutation(case.E)), case.name


# mutant -> (kind, dtype, random perm, layouts that must each expose it, layouts that cannot)
PLANTED = {
    'no_max': ('big', 'f32', False, ('hub', 'lengths', 'single'), ()),
    'per_chunk': ('normal', 'f32', False, ('hub', 'boundaries', 'lengths'), ('single', )),
    'no_rescale': ('late_max', 'f32', False, ('hub', 'boundaries'), ('single', )),
    'unguarded_identity': ('neg_inf_piece', 'f32', False, ('hub', ), ('single', )),
    'perm_read_only': ('normal', 'f32', True, ('lengths', 'empties', 'hub'), ()),
    'shared_normaliser': ('normal', 'f32', False, ('lengths', 'hub', 'empties'), ()),
    'storage_sum': ('normal', 'bf16', False, ('hub', ), ('single', )),
    'bw_no_dot': ('normal', 'f32', False, ('lengths', 'hub', 'empties'), ()),
}


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_comparators_reject_planted_defect(mutant):
    kind, dtype, shuffled, exposed, blind = PLANTED[mutant]
    for name in exposed + blind:
        case = BY_NAME[name]
        perm = np.random.default_rng(4).permutation(case.E) if shuffled else None
        assert _accepts(case, kind, dtype, None, perm), 'the unplanted softmax on %s' % name
        assert _accepts(case, kind, dtype, mutant, perm) == (name in blind), '%s on %s' % (mutant, name)


def test_planted_defects_cover_the_list():
    assert sorted(PLANTED) == sorted(R.MUTANTS) and len(R.MUTANTS) == 8


def test_entry_status_codes_before_any_device_call():
    """tsamd_segment_softmax / _bw validate in this order, all on the host; route and workspace_bytes are arithmetic."""
    L = nat.lib()
    i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    fake = vp(0x1000)  # never dereferenced
    INVALID, UNSUPPORTED, WORKSPACE, OK = 1, 2, 4, 0

    def fw(dtype=0, nseg=3, E=4, D=1, value=fake, out=fake, ptr=fake, ws=fake, nbytes=1 << 20):
        return L.tsamd_segment_softmax(dtype, value, None, ptr, i64(nseg), i64(E), i64(D), out, ws, sz(nbytes), None)

    def bw(dtype=0, nseg=3, E=4, D=1, y=fake, grad=fake, out=fake, ptr=fake, ws=fake, nbytes=1 << 20):
        return L.tsamd_segment_softmax_bw(dtype, y, grad, None, ptr, i64(nseg), i64(E), i64(D), out, ws, sz(nbytes),
                                          None)

    for call in (fw, bw):
        assert call(nseg=-1) == INVALID and call(E=-1) == INVALID and call(D=-1) == INVALID
        for dt in (4, 5, 6, 7, 8, 9, -1):  # the integers, unknown codes
            assert call(dtype=dt) == UNSUPPORTED
        assert call(D=65536) == UNSUPPORTED
        assert call(nseg=-1, dtype=5) == INVALID, 'a negative size wins over the dtype'
        assert call(E=0, out=None, ptr=None, ws=None, nbytes=0) == OK
        assert call(D=0, out=None, ptr=None, ws=None, nbytes=0) == OK
        assert call(E=0, dtype=5) == UNSUPPORTED, 'the dtype is checked before the empty call returns'
        assert call(out=None) == INVALID and call(ptr=None) == INVALID and call(nseg=0) == INVALID
        assert call(ws=None) == WORKSPACE and call(nbytes=255) == WORKSPACE
        assert call(out=None, ws=None) == INVALID, 'a null pointer wins over the workspace'
    assert fw(value=None) == INVALID and bw(y=None) == INVALID and bw(grad=None) == INVALID
    assert b'workspace' in L.tsamd_status_string(WORKSPACE)

    ws = L.tsamd_segment_softmax_workspace_bytes
    chunk = R.CHUNK
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    for dt, acc in ((0, 4), (1, 8), (2, 4), (3, 4)):
        for E, D in ((1, 1), (chunk, 1), (chunk + 1, 1), (70_000, 3), (1 << 21, 8)):
            nch = -(-E // chunk)
            assert ws(dt, i64(E), i64(D)) == 3 * a256(2 * acc * D * nch) + 2 * a256(8 * nch), (dt, E, D)
        assert ws(dt, i64(0), i64(0)) == ws(dt, i64(1), i64(1))
    assert ws(5, i64(100), i64(1)) == 0 and ws(42, i64(100), i64(1)) == 0
    assert L.tsamd_segment_softmax_route(None) == INVALID
    assert R.route() == (512, 2048, 2048, 64)
