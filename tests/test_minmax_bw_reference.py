"""tests/minmax_bw_reference.py held to independent statements of the same things, without a GPU: its gradients to
torch's fp64 autograd of the gather form and to the C oracle, its records to the properties of the layout, its builders
to the census they claim (the builders assert it themselves; building them is the test), the route query of the
min / max backward to literals at every threshold, and its comparators to twelve planted defects -- each must be
rejected bit for bit AND by the derived bounds -- while a plain restatement of each route's arithmetic stays inside them."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle as oc
from pytorch_sparse_amd import _native as nat
from tests import minmax_bw_reference as mr
from tests import spmm_forward_reference as fr

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


def _scatter_route(K, dtype=BF16, **kw):
    return nat.spmm_minmax_bw_route('none', dtype, 1, 100, 100, K, 1000, True, True, **kw)


@functools.lru_cache(maxsize=None)
def _row_parallel(K, dtype, exact, reduce='max', B=None):
    return mr.build_row_parallel(K, _scatter_route(K, dtype), dtype, reduce, True, exact, seed=K, B=B)


def _fw_route(dtype, K, M, E, B=1):
    return nat.spmm_route(dtype, 'max', B, M, E + 2, K, E, arg32=True)


@functools.lru_cache(maxsize=None)
def _record_forward(K, dtype, exact, B=None, long_rows=(1025, 3001), long_winners=mr.LONG_WINNERS):
    # (items and snap do not move with M and E at this scale; the case is rebuilt should they)
    route = _fw_route(dtype, K, 100, 30000)
    c = mr.build_record_forward(K, route, dtype, 'max', True, exact, seed=3, B=B, long_rows=long_rows,
                                long_winners=long_winners)
    again = _fw_route(dtype, K, c.M, c.E, c.B)
    assert (again['items'], again['snap']) == (route['items'], route['snap'])
    return c


# ---- the gradients -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('has_value', [True, False])
@pytest.mark.parametrize('B', [None, 2])
def test_grads_against_autograd_and_the_c_oracle(has_value, B):
    c = mr.build_small(7, 5, 9, F64, 'max', has_value, exact=False, seed=4, B=B, deg=4)
    loops = mr.grads_loops(c.rowptr, c.col, c.value, c.x, c.gout, c.arg, has_value)
    vec = c.ref
    for key in loops:
        if loops[key] is None:
            assert vec[key] is None
        else:
            assert np.allclose(np.asarray(vec[key], np.float64), loops[key], rtol=1e-15, atol=0), key
    # torch: out = value[arg] * x[col[arg]] gathered (no amax: its tie rule differs), loss = sum(out * g)
    x = torch.from_numpy(np.nan_to_num(c.x)).requires_grad_()
    v = torch.from_numpy(c.value).requires_grad_() if has_value else None
    arg = torch.from_numpy(np.asarray(c.arg))
    ok = arg != c.E
    a = torch.where(ok, arg, 0)
    xg = torch.gather(x, -2, torch.from_numpy(c.col)[a])  # xg[.., m, k] = x[.., col[arg[.., m, k]], k]
    out = (v[a] * xg) if has_value else xg
    (torch.where(ok, out, 0.0) * torch.from_numpy(c.gout)).sum().backward()
    assert np.allclose(x.grad.numpy(), np.asarray(vec['gm'], np.float64), rtol=1e-13, atol=1e-13)
    if has_value:
        assert np.allclose(v.grad.numpy(), np.asarray(vec['gv'], np.float64), rtol=1e-13, atol=1e-13)
    gv, gm = oc.spmm_minmax_bw(oc.F64, c.col, c.value, np.nan_to_num(c.x), c.gout, c.arg, want_value=has_value)
    assert np.allclose(gm, np.asarray(vec['gm'], np.float64), rtol=1e-13, atol=1e-13)
    if has_value:
        assert np.allclose(gv, np.asarray(vec['gv'], np.float64), rtol=1e-13, atol=1e-13)


def test_loops_equal_the_vectorised_form_on_a_builder():
    c = _row_parallel(4, BF16, True)
    loops = mr.grads_loops(c.rowptr, c.col, c.value, c.x, c.gout, c.arg, True)
    for key, want in loops.items():
        assert np.array_equal(np.asarray(c.ref[key], np.float64), want), key


# ---- the records -------------------------------------------------------------------------------------------------
STRIDES = {32: (1, 4), 33: (2, 8), 64: (2, 8), 96: (3, 8), 100: (4, 8), 128: (4, 8), 132: (5, 8), 160: (5, 8), 161: (6, 12),
           256: (8, 12), 260: (9, 12), 288: (9, 12), 1024: (32, 36), 1056: (33, 36), 1088: (34, 40)}
NO_BITMAP_WORD = (32, 132, 160, 260, 288, 1056)  # W = 1, 5, 9, 33: W + 3 is a multiple of 4


@pytest.mark.parametrize('K', mr.W_LADDER)
def test_record_layout_at_every_width(K):
    assert mr.record_words(K) == STRIDES[K]
    W, S = STRIDES[K]
    d = mr.defined_words(K)
    assert d.sum() == W + 3 + (0 if K in NO_BITMAP_WORD else 1) and d[:W + 3].all() and not d[W + 4:].any()
    assert mr.masked_has_z(K) == (K not in NO_BITMAP_WORD and W <= 32)
    r = nat.spmm_minmax_bw_route('records', F32, 1, 50, 50, K, 300)
    assert (r['W'], r['S'], r['has_z']) == (W, S, int(mr.masked_has_z(K)))
    for dtype, B in ((F32, None), (F64, 2)):
        c = mr.tiny_case(K, dtype, 'max', True, exact=False, seed=K, B=B, plant_high=K > 1024)
        rec = c.rec
        assert rec.shape == (c.B, c.E, S) and rec.dtype == np.uint32
        arg, claims = mr.decode(rec, K, c.M)
        assert np.array_equal(arg.reshape(np.shape(c.arg)), c.arg) and claims <= 1
        bits = mr.mask_bits(rec, K)
        per_row = np.zeros((c.B, c.M, K), np.int64)
        for b in range(c.B):
            np.add.at(per_row[b], c.row, bits[b].astype(np.int64))
        assert np.array_equal(per_row, (mr._b3(c.arg, np.int64) != c.E).astype(np.int64))
        assert (rec[:, :, W] == c.row[None]).all()
        if W + 3 < S and d[W + 3]:
            want = sum(((rec[:, :, s] != 0).astype(np.uint32) << np.uint32(s)) for s in range(min(W, 32)))
            assert np.array_equal(rec[:, :, W + 3], want)
        vals = mr.record_values(rec, K, dtype)
        assert np.array_equal(vals, np.broadcast_to(c.value, vals.shape))
        if dtype == F64:
            both = rec[0, :, W + 1].astype(np.uint64) | (rec[0, :, W + 2].astype(np.uint64) << np.uint64(32))
            assert np.array_equal(both, c.value.view(np.uint64)) and (rec[:, :, W + 2] != 0).all()
        else:
            assert (rec[:, :, W + 2] == 0).all()
    c = mr.tiny_case(K, BF16, 'min', False, exact=True, seed=1)
    assert (c.rec[:, :, W + 1] == 0x3F800000).all()  # 1.0 without values


# ---- the route query ---------------------------------------------------------------------------------------------
def test_route_scatter_lane_groups_and_capacity():
    want = {64: (0, 256), 32: (1, 128), 16: (2, 64), 8: (3, 32), 4: (4, 16), 2: (5, 8), 1: (6, 4), 65: (0, 256),
            127: (0, 256), 129: (0, 256), 33: (0, 256), 17: (1, 128), 3: (4, 16)}
    for K, (lgG, cap) in want.items():
        r = _scatter_route(K, F32)
        assert (r['status'], r['value'], r['mat'], r['lgG'], r['cap']) == (OK, 'row_parallel', 'scatter', lgG, cap), K
        assert (r['packed'], r['shadow'], r['shadow_bytes']) == ('plain', 0, 0)
        assert lgG == mr.scatter_lgG(K)
    assert _scatter_route(64, F32)['W'] == 0 and _scatter_route(64, F32)['items'] == 0


def test_route_packed_and_shadow():
    q = lambda dtype, N, K, **kw: nat.spmm_minmax_bw_route('none', dtype, 1, 9, N, K, 20, True, True, **kw)  # noqa: E731
    for dtype in (BF16, F16):
        assert (q(dtype, 5, 4)['packed'], q(dtype, 5, 4)['shadow']) == ('merge_pairs', 0)
        assert (q(dtype, 6, 3)['packed'], q(dtype, 6, 3)['shadow']) == ('idx_parity', 0)   # odd K, even count
        r = q(dtype, 5, 3)                                                                 # 15 elements
        assert (r['packed'], r['shadow'], r['shadow_bytes']) == ('plain', 1, 256)
        r = q(dtype, 5, 4, grad_mat=0x1002)                                                # even count, 2 bytes in
        assert (r['packed'], r['shadow'], r['shadow_bytes']) == ('plain', 1, 256)
        assert q(dtype, 5, 4, grad_mat=0x1004)['shadow'] == 0
        assert q(dtype, 65, 65)['shadow_bytes'] == 16896 + 256 - 16896 % 256                # 4 * 4225 rounded up to 256
        lib = nat.lib()
        i64 = nat._i64
        assert lib.tsamd_spmm_minmax_bw_workspace_bytes(nat.dtype_code(dtype), i64(1), i64(65), i64(65), i64(20)) == 17152
    for dtype in (F32, F64):
        assert (q(dtype, 5, 3)['packed'], q(dtype, 5, 3)['shadow']) == ('plain', 0)
    # grad_mat only / grad_value only / nothing
    r = nat.spmm_minmax_bw_route('none', BF16, 1, 9, 5, 4, 20, False, True)
    assert (r['value'], r['mat']) == ('none', 'scatter')
    r = nat.spmm_minmax_bw_route('none', BF16, 1, 9, 5, 3, 20, True, False)
    assert (r['value'], r['mat'], r['shadow']) == ('row_parallel', 'none', 0)
    r = nat.spmm_minmax_bw_route('none', BF16, 1, 9, 5, 3, 20, False, False)
    assert (r['status'], r['value'], r['mat']) == (OK, 'none', 'none')


def test_route_pull_sixteen_byte_rule():
    q = lambda w, K, dtype=BF16, **kw: nat.spmm_minmax_bw_route(w, dtype, 1, 1000, 1000, K, 20000, True, True, **kw)  # noqa: E731
    for w in ('ids64', 'ids32', 'records'):
        r = q(w, 64)
        assert (r['status'], r['value'], r['sddmm'], r['mat'], r['write_records']) == \
            (OK, 'masked_sddmm', 'pipelined', 'pull', 0 if w == 'records' else 1), w
        assert q(w, 64, mat=0x1010)['value'] == 'masked_sddmm' and q(w, 64, grad_out=0x2000)['value'] == 'masked_sddmm'
    for kw in (dict(mat=0x1008), dict(grad_out=0x1008), dict(mat=0x1008, grad_out=0x1008)):
        r = q('ids64', 64, **kw)
        assert (r['status'], r['value'], r['mat'], r['lgG'], r['cap']) == (OK, 'row_parallel', 'pull', 0, 256)
        assert q('ids32', 64, **kw)['status'] == UNSUPPORTED and q('records', 64, **kw)['status'] == UNSUPPORTED
    # K * es % 16: bf16 K = 36 is 72 bytes a row, 40 is 80
    assert q('ids64', 36)['value'] == 'row_parallel' and q('ids64', 40)['value'] == 'masked_sddmm'
    assert q('ids32', 36)['status'] == UNSUPPORTED and q('records', 36)['status'] == UNSUPPORTED
    assert q('ids64', 2, F64)['value'] == 'masked_sddmm' and q('ids64', 3, F64)['value'] == 'row_parallel'
    assert q('ids64', 4, F32)['value'] == 'masked_sddmm' and q('ids64', 6, F32)['value'] == 'row_parallel'
    # packets per row: 64 keeps the pipelined kernel, 65 takes the other one
    for dtype, vec in ((BF16, 8), (F16, 8), (F32, 4), (F64, 2)):
        for packets, lgG in ((1, 6), (2, 5), (3, 4), (4, 4), (8, 3), (16, 2), (24, 1), (32, 1), (64, 0)):
            r = q('ids32', packets * vec, dtype)
            assert (r['sddmm'], r['sddmm_lgG']) == ('pipelined', lgG), (dtype, packets)
        assert q('ids32', 65 * vec, dtype)['sddmm'] == 'round4' and q('ids32', 65 * vec, dtype)['sddmm_lgG'] == 0
    # without grad_value nothing of this matters
    r = nat.spmm_minmax_bw_route('records', BF16, 1, 1000, 1000, 36, 20000, False, True, mat=0x1008)
    assert (r['status'], r['value'], r['mat'], r['write_records']) == (OK, 'none', 'pull', 0)


def test_route_pull_masked_sum_words():
    r = nat.spmm_minmax_bw_route('records', BF16, 1, 1000, 1000, 128, 20000, True, True)
    f = nat.spmm_route(BF16, 'sum', 1, 1000, 1000, 128, 20000)
    assert (r['items'], r['P'], r['fixup'], r['vec'], r['lpr'], r['sum_lgG'], r['ktiles'], r['family']) == \
        (f['items'], f['P'], f['fixup'], f['vec'], f['lpr'], f['lgG'], f['ktiles'], f['family'])
    assert (r['items'], r['P'], r['fixup'], r['vec'], r['lpr'], r['sum_lgG'], r['ktiles']) == (128, 165, 1, 4, 32, 1, 1)
    assert (r['workspace_bytes'], nat.spmm_minmax_bw_route('ids64', BF16, 1, 1000, 1000, 128, 20000)['workspace_bytes']) == \
        (175104, 815104)  # (tests/test_cabi_minmax_bw.py pins the same two)
    # the transposed problem: N rows.  Where the forward would probe the ids (relabel 2) the masked sum copies (1)
    f = nat.spmm_route(BF16, 'sum', 1, 8192, 4096, 128, 1 << 20)
    r = nat.spmm_minmax_bw_route('ids32', BF16, 1, 4096, 8192, 128, 1 << 20)
    assert f['relabel'] == 2 and (r['relabel'], r['copy']) == (1, 1) and r['P'] == f['P']
    # a misaligned grad_out narrows the packets of the sum
    assert nat.spmm_minmax_bw_route('ids64', BF16, 1, 1000, 1000, 128, 20000, False, True, grad_out=0x1004)['vec'] == 2


def test_route_status_rows():
    q = nat.spmm_minmax_bw_route
    big = dict(B=1, M=8, N=8, K=64, E=16)
    call = lambda w, wv=False, wm=True, dtype=BF16, **kw: q(w, dtype, *[{**big, **kw}[k] for k in 'BMNKE'], wv, wm)  # noqa: E731
    for w in ('ids64', 'ids32', 'records'):
        assert call(w, M=-1)['status'] == INVALID
        assert call(w, dtype=4)['status'] == UNSUPPORTED
        for kw in (dict(N=1 << 32), dict(M=1 << 32), dict(E=1 << 32), dict(K=1 << 31)):
            assert call(w, **kw)['status'] == UNSUPPORTED, (w, kw)
        r = call(w, N=0)
        assert (r['status'], r['value'], r['mat']) == (OK, 'none', 'none')
        r = call(w, E=0)
        assert (r['status'], r['mat']) == (OK, 'zero')
        r = call(w, M=0, wv=True)
        assert (r['status'], r['mat'], r['value']) == (OK, 'zero', 'zero')
    # E = 2^31: the two 32-bit kinds end there, the int64 entry goes on
    assert call('ids32', E=1 << 31)['status'] == UNSUPPORTED and call('records', E=1 << 31)['status'] == UNSUPPORTED
    assert call('ids64', E=1 << 31)['status'] == OK and call('ids64', E=(1 << 31) - 1)['status'] == OK
    assert call('ids32', E=(1 << 31) - 1)['status'] == OK
    # the table's rows without grad_mat
    assert call('records', wm=False)['status'] == UNSUPPORTED and call('records', wv=True, wm=False)['status'] == UNSUPPORTED
    assert call('ids32', wv=True, wm=False)['status'] == UNSUPPORTED
    r = call('ids64', wv=True, wm=False)
    assert (r['status'], r['value'], r['mat']) == (OK, 'row_parallel', 'none')
    r = call('ids32', wm=False)
    assert (r['status'], r['value'], r['mat']) == (OK, 'none', 'none')
    # the bare scatter entry
    assert call('none', M=-1)['status'] == INVALID and call('none', dtype=5)['status'] == UNSUPPORTED
    assert call('none', N=1 << 32)['status'] == UNSUPPORTED and call('none', M=1 << 32)['status'] == OK
    r = call('none', wv=True, M=0)
    assert (r['status'], r['value'], r['mat']) == (OK, 'zero', 'zero')
    # B * N * K == 0 with E > 0 and both gradients: OK, and grad_value is not made (the open point of the design page)
    r = call('records', wv=True, K=0)
    assert (r['status'], r['value'], r['mat']) == (OK, 'none', 'none')
    words = (nat.ctypes.c_int64 * 32)()
    assert nat.lib().tsamd_spmm_minmax_bw_route(7, 0, *[nat._i64(1)] * 5, 0, 0, None, None, None, words) == INVALID
    assert nat.lib().tsamd_spmm_minmax_bw_route(0, 0, *[nat._i64(1)] * 5, 0, 0, None, None, None, None) == INVALID


# ---- the builders' censuses ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [64, 32, 16, 8, 4, 2, 1, 65, 127, 129])
def test_row_parallel_builder_census(K):
    for dtype, exact in ((BF16, True), (F32, False)):
        c = _row_parallel(K, dtype, exact)
        assert c.E < 10 ** 5 and c.N * K < 10 ** 6
        assert c.census['passes'] >= 3 and c.M % c.census['per_wave'] != 0
        if exact:
            mr.assert_exact_mode(c.ref, dtype)


@pytest.mark.parametrize('K,dtype', [(128, BF16), (100, F16), (64, BF16), (256, F32), (132, BF16)])
def test_record_forward_builder_census(K, dtype):
    route = _fw_route(dtype, K, 100, 30000)
    assert route['records'] == (1 if 97 <= K <= 128 else 2) and route['snap'] == min(128, route['items'] // 2)
    c = _record_forward(K, dtype, False)
    assert c.distinct['long1025_63'] == 63 and c.distinct['long3001_65'] == min(65, K) and c.distinct['long1025_none'] == 0
    assert c.distinct['long3001_K'] == K and c.distinct['long1025_one'] == 1
    assert c.E < 10 ** 5 and c.M * K < 10 ** 6
    rel = c.rel()[0]
    for d in (1025, 3001):
        m = c.named['long%d_K' % d]
        assert 0 in rel[m] and d - 1 in rel[m] and 4 in rel[m] and 5 in rel[m], 'first / last entry of the row and of a piece'


def test_masked_sum_builder_census():
    r = nat.spmm_minmax_bw_route('records', BF16, 1, 3000, 600, 128, 60000)
    c = mr.build_masked_sum(r['items'], 128, BF16, exact=False, seed=0)
    again = nat.spmm_minmax_bw_route('records', BF16, 1, c.M, c.N, 128, c.E)
    assert again['items'] == r['items'] and again['fixup'] == 1
    colptr, _ = c.csc()
    got = fr.census(colptr, fr.partition(colptr, r['items'], 0), r['items'])
    for run in c.keys['run_hist']:
        assert got['run_hist'].get(run, 0) >= 1, run
    assert got['cut_last_row'] == 1 and got['empty_head'] >= 1
    assert c.E < 10 ** 5 and c.N * 128 < 10 ** 6
    # a 32-feature segment without any winner next to one with exactly one
    words = c.rec[0, :, :4]
    pop = np.zeros(words.shape, np.int64)
    for s in range(32):
        pop += (words >> np.uint32(s)) & 1
    assert ((pop == 0).any(axis=1) & (pop == 1).any(axis=1)).any()


# ---- planted defects -----------------------------------------------------------------------------------------------
def _reject(c, gm=None, gv=None, mat_bound=None, exact=True):
    """-> True when the comparator of the case's mode rejects the gradients"""
    ref = c.ref
    bad = 0
    if exact:
        mr.assert_exact_mode(ref, c.dtype)
        if gm is not None:
            bad += mr.exact_mismatches(gm, ref['gm'], c.dtype)
        if gv is not None:
            bad += mr.exact_mismatches(gv, ref['gv'], c.dtype)
        return bad > 0
    if gm is not None:
        bound = mr.bound_scatter_mat(ref['gm_l1'], ref['gm_n'], c.dtype) if mat_bound == 'scatter' else \
            mr.bound_pull_mat(ref['gm'], ref['gm_l1'], ref['gm_n'], c.dtype)
        bad += mr.violations(gm, ref['gm'], bound, c.dtype)[0]
    if gv is not None:
        bad += mr.violations(gv, ref['gv'], mr.bound_value(ref['gv'], ref['gv_l1'], c.dtype, c.B * c.K), c.dtype)[0]
    return bad > 0


@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
@pytest.mark.parametrize('defect', mr.DEFECTS)
def test_planted_defects_are_rejected(defect, exact):
    if defect in ('winner_at_cap_lost', 'odd_half_added_to_even', 'zero_mate_replaced', 'tie_to_larger_id'):
        c = _row_parallel(8, BF16, exact) if defect != 'tie_to_larger_id' else \
            mr.build_small(6, 4, 40, BF16, 'max', True, True, seed=2, deg=6)  # integers: ties abound
        if defect == 'tie_to_larger_id':
            if not exact:  # real gradients on the same tied winners
                c.gout = fr.rounded(np.random.default_rng(1).standard_normal(c.gout.shape), BF16)
                c._ref = None
            assert not np.array_equal(mr.tie_to_larger_id(c), c.arg)
            gm, gv = mr.restate_scatter(c, arg=mr.tie_to_larger_id(c))
        else:
            gm, gv = mr.restate_scatter(c, defect=defect, cap=_scatter_route(8)['cap'])
        good = mr.restate_scatter(c)
        assert not _reject(c, *good, mat_bound='scatter', exact=exact)
        assert _reject(c, gm, gv, mat_bound='scatter', exact=exact)
        return
    if defect == 'inf_times_zero':
        c = mr.tiny_case(64, BF16, 'max', True, exact, seed=5)
        a = mr._b3(c.arg, np.int64)[0]
        m = 1  # the 70-entry row: most of its entries lose feature 0
        assert (a[m] != c.E).all()
        c.gout[m, 0] = np.inf
        c._ref = None
        good = mr.restate_pull(c, c.rec)
        bad = mr.restate_pull(c, c.rec, defect)
        # only the winner of (m, 0) sees the Inf; the defect gives every other entry of the row a NaN
        assert np.isinf(np.asarray(c.ref['gv'], np.float64)).sum() == 1
        assert int(torch.isnan(bad[1]).sum()) >= 60 and int(torch.isnan(good[1]).sum()) == 0
        keep = np.isfinite(np.asarray(c.ref['gv'], np.float64))
        if exact:
            assert mr.exact_mismatches(good[1][keep], c.ref['gv'][keep], BF16) == 0
            assert mr.exact_mismatches(bad[1][keep], c.ref['gv'][keep], BF16) > 0
        else:
            bound = mr.bound_value(c.ref['gv'], c.ref['gv_l1'], BF16, c.K)[keep]
            assert mr.violations(good[1][keep], c.ref['gv'][keep], bound, BF16)[0] == 0
            assert mr.violations(bad[1][keep], c.ref['gv'][keep], bound, BF16)[0] > 0
        return
    kw = {}
    if defect == 'bitmap_from_four_words':
        c = mr.tiny_case(256, BF16, 'max', True, exact, seed=6)
        assert mr.record_words(256)[0] == 8
    elif defect == 'bitmap_honoured_beyond_32_words':
        c = mr.tiny_case(1088, F32, 'max', True, exact, seed=6, plant_high=True)
    elif defect == 'value_as_element_bits':
        c = mr.tiny_case(64, BF16, 'max', True, exact, seed=6)
    elif defect == 'empty_column_unwritten':
        c = mr.tiny_case(64, BF16, 'max', True, exact, seed=6)
        assert (np.bincount(c.col, minlength=c.N) == 0).any()
    elif defect == 'blank_last_record_of_rewrite':
        c = _record_forward(64, BF16, exact, long_rows=(), long_winners=())
        kw = dict(rewrite_rows=[c.named['rewrite193']])
    elif defect == 'walk_stops_at_64':
        c = _record_forward(128, F32, exact, long_rows=(1025, ), long_winners=(65, ))
        kw = dict(long_rows=[c.named['long1025_65']])
    elif defect == 'batch1_not_rewritten':
        c = _record_forward(64, BF16, exact, B=2, long_rows=(1025, ), long_winners=(64, ))
        kw = dict(long_rows=[c.named['long1025_64']])
    rec = mr.restate_records(c, defect, **kw)
    reader = defect if defect in ('bitmap_honoured_beyond_32_words', 'empty_column_unwritten') else None
    if reader is None:
        assert mr.record_mismatches(rec, c.rec, c.K) > 0 and mr.record_mismatches(c.rec.copy(), c.rec, c.K) == 0
    assert not _reject(c, *mr.restate_pull(c, c.rec), exact=exact)
    assert _reject(c, *mr.restate_pull(c, rec, reader), exact=exact)


# ---- the plain restatements stay inside the bounds ---------------------------------------------------------------
# worst error / bound of the numpy restatements on the widest builders, measured here and rounded up to two digits
CEILINGS = {('pull_mat', BF16): 0.77, ('pull_mat', F16): 0.77, ('pull_mat', F32): 0.30,
            ('value', BF16): 0.99, ('value', F16): 0.96, ('value', F32): 0.013,
            ('scatter_mat', BF16): 0.33, ('scatter_mat', F16): 0.34, ('shadow_mat', BF16): 0.50, ('shadow_mat', F16): 0.50}


def plain_ratios():
    out = {}
    for dtype in (BF16, F16, F32):
        r = nat.spmm_minmax_bw_route('records', dtype, 1, 3000, 600, 128, 60000)
        c = mr.build_masked_sum(r['items'], 128, dtype, exact=False, seed=1)
        gm, gv = mr.restate_pull(c, c.rec)
        ref = c.ref
        out[('pull_mat', dtype)] = mr.violations(gm, ref['gm'], mr.bound_pull_mat(ref['gm'], ref['gm_l1'], ref['gm_n'], dtype), dtype)
        out[('value', dtype)] = mr.violations(gv, ref['gv'], mr.bound_value(ref['gv'], ref['gv_l1'], dtype, 128), dtype)
        if dtype == F32:
            continue
        c = _row_parallel(129, dtype, False)
        ref = c.ref
        gm, _ = mr.restate_scatter(c)
        out[('scatter_mat', dtype)] = mr.violations(gm, ref['gm'], mr.bound_scatter_mat(ref['gm_l1'], ref['gm_n'], dtype), dtype)
        gm, gv = mr.restate_scatter(c, shadow=True)
        out[('shadow_mat', dtype)] = mr.violations(gm, ref['gm'], mr.bound_shadow_mat(ref['gm'], ref['gm_l1'], ref['gm_n'], dtype), dtype)
        worse = mr.violations(gv, ref['gv'], mr.bound_value(ref['gv'], ref['gv_l1'], dtype, 129), dtype)
        out[('value', dtype)] = max(out[('value', dtype)], worse, key=lambda t: t[1])
    return out


def test_plain_restatements_stay_inside_the_bounds():
    got = plain_ratios()
    assert set(got) == set(CEILINGS)
    for key, (bad, ratio) in got.items():
        assert bad == 0 and ratio <= 1.0, (key, bad, ratio)
        assert ratio <= CEILINGS[key], (key, ratio)
