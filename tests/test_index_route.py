"""The sizes at which the index kernels change route (tsamd_index_route: csrc/scan.hip, convert.hip, expand.h,
select.hip), pinned as literals on purpose -- whoever moves a tile size or the long-run threshold revisits the cases of
tests/index_reference.py knowingly -- and the status code of every index entry point for every argument combination it
refuses.  Host arithmetic and validation only: every refused call returns before any HIP call, `fake` is never
dereferenced; runs without a GPU."""
import ctypes

import pytest

from pytorch_sparse_amd import _native as nat

i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
fake = vp(0x1000)
BIG = sz(1 << 40)
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


def test_index_route_values():
    out = (ctypes.c_int64 * 8)(*([-7] * 8))
    assert nat.lib().tsamd_index_route(out) == OK
    assert list(out) == [2048, 2048, 2048, 256, 1024, 0, 0, 0]
    assert nat.lib().tsamd_index_route(None) == INVALID


def test_num_diag_is_host_arithmetic():
    L = nat.lib()
    assert [L.tsamd_num_diag(i64(3), i64(5), i64(k)) for k in range(-4, 7)] == [0, 0, 1, 2, 3, 3, 3, 2, 1, 0, 0]
    assert [L.tsamd_num_diag(i64(5), i64(3), i64(k)) for k in range(-6, 5)] == [0, 0, 1, 2, 3, 3, 3, 2, 1, 0, 0]
    assert L.tsamd_num_diag(i64(0), i64(4), i64(0)) == 0 and L.tsamd_num_diag(i64(4), i64(0), i64(0)) == 0


def _scan(inp=fake, out=fake, n=5000, total=fake, ws=fake, wsb=BIG):
    return nat.lib().tsamd_exclusive_scan_i64(inp, out, i64(n), total, ws, wsb, None)


def test_status_scan():
    L = nat.lib()
    assert _scan(n=-1) == INVALID and _scan(inp=None) == INVALID and _scan(out=None) == INVALID
    assert _scan(inp=None, n=5) == INVALID and _scan(out=None, n=5) == INVALID
    need = L.tsamd_exclusive_scan_workspace_bytes(i64(5000))
    assert _scan(ws=None) == WORKSPACE and _scan(ws=None, wsb=sz(0)) == WORKSPACE and _scan(wsb=sz(need - 1)) == WORKSPACE
    need3 = L.tsamd_exclusive_scan_workspace_bytes(i64(2048 * 2048 + 1))
    assert _scan(n=2048 * 2048 + 1, wsb=sz(need3 - 1)) == WORKSPACE      # the third level counts
    assert _scan(n=0, inp=None, out=None, total=None, ws=None, wsb=sz(0)) == OK   # nothing to do, nothing touched


def test_status_ind2ptr_ptr2ind():
    L = nat.lib()
    assert L.tsamd_ind2ptr(fake, i64(-1), i64(3), fake, None) == INVALID
    assert L.tsamd_ind2ptr(fake, i64(4), i64(-1), fake, None) == INVALID
    assert L.tsamd_ind2ptr(fake, i64(4), i64(3), None, None) == INVALID
    assert L.tsamd_ind2ptr(None, i64(4), i64(3), fake, None) == INVALID
    assert L.tsamd_ind2ptr(None, i64(4), i64(0), None, None) == INVALID       # out is written even for E = 0
    assert L.tsamd_ptr2ind(fake, i64(-1), i64(3), fake, None) == INVALID
    assert L.tsamd_ptr2ind(fake, i64(4), i64(-1), fake, None) == INVALID
    assert L.tsamd_ptr2ind(None, i64(4), i64(3), fake, None) == INVALID
    assert L.tsamd_ptr2ind(fake, i64(4), i64(3), None, None) == INVALID
    assert L.tsamd_ptr2ind(fake, i64(4), i64(0), None, None) == OK
    assert L.tsamd_ptr2ind(fake, i64(0), i64(3), fake, None) == OK


def _plan(ptr=fake, S=10, idx=fake, K=5, out_ptr=fake, info=fake, ws=fake, wsb=BIG):
    return nat.lib().tsamd_select_plan(ptr, i64(S), idx, i64(K), out_ptr, info, ws, wsb, None)


def _fill(ptr=fake, S=10, ind=fake, idx=fake, K=5, out_ptr=fake, total=7, seg=fake, ind_out=fake, pos=fake):
    return nat.lib().tsamd_select_fill(ptr, i64(S), ind, idx, i64(K), out_ptr, i64(total), seg, ind_out, pos, None)


def test_status_select():
    L = nat.lib()
    assert _plan(S=-1) == INVALID and _plan(K=-1) == INVALID
    assert _plan(ptr=None) == INVALID and _plan(idx=None) == INVALID
    assert _plan(out_ptr=None) == INVALID and _plan(info=None) == INVALID
    assert _plan(out_ptr=None, K=0) == INVALID and _plan(info=None, K=0) == INVALID
    for K in (0, 5, 5000, 2048 * 2048):
        need = L.tsamd_select_workspace_bytes(i64(K))
        assert need >= 256
        assert _plan(K=K, ws=None) == WORKSPACE and _plan(K=K, ws=None, wsb=sz(0)) == WORKSPACE
        assert _plan(K=K, wsb=sz(need - 1)) == WORKSPACE
    assert _fill(S=-1) == INVALID and _fill(K=-1) == INVALID and _fill(total=-1) == INVALID
    assert _fill(ptr=None) == INVALID and _fill(idx=None) == INVALID and _fill(out_ptr=None) == INVALID
    assert _fill(ind=None) == INVALID                                         # ind_out wants ind
    assert _fill(K=0, ptr=None, idx=None, out_ptr=None) == OK and _fill(total=0, ptr=None, idx=None, out_ptr=None) == OK


NEEDS = {0: ('col', ), 1: ('row', 'col'), 2: ('mask', ), 3: ('row', 'mask'), 4: ('col', 'mask'), 5: ('col', 'map')}


def _fplan(pred=0, row=fake, col=fake, mask=fake, map=fake, n=5000, pos=fake, count=fake, ws=fake, wsb=BIG):
    return nat.lib().tsamd_filter_plan(pred, row, col, mask, map, i64(n), i64(0), i64(3), pos, count, ws, wsb, None)


def _fcount(pred=0, row=fake, col=fake, mask=fake, map=fake, n=5000, count=fake, ws=fake, wsb=BIG):
    return nat.lib().tsamd_filter_count(pred, row, col, mask, map, i64(n), i64(0), i64(3), count, ws, wsb, None)


def _fwrite(pred=0, row=fake, col=fake, mask=fake, map=fake, n=5000, ws=fake, row_out=fake, col_out=fake, src_out=fake):
    return nat.lib().tsamd_filter_write(pred, row, col, mask, map, i64(n), i64(0), i64(3), ws, None, None, i64(0), i64(0),
                                        row_out, col_out, src_out, None)


def _fapply(pos=fake, row=fake, col=fake, n=5000, row_out=fake, col_out=fake, src_out=fake):
    return nat.lib().tsamd_filter_apply(pos, row, col, i64(n), None, None, i64(0), i64(0), row_out, col_out, src_out, None)


@pytest.mark.parametrize('pred', range(6))
def test_status_filter(pred):
    L = nat.lib()
    for f in (_fplan, _fcount, _fwrite):
        assert f(pred=pred, n=-1) == INVALID
        for name in ('row', 'col', 'mask', 'map'):
            want = INVALID if name in NEEDS[pred] else None
            got = f(pred=pred, **{name: None, 'ws': None} if want is None else {name: None})
            # an input the predicate does not read may be NULL: the call goes on to the next check (the workspace)
            assert got == (want if want is not None else (INVALID if f is _fwrite else WORKSPACE)), (f.__name__, name)
    assert _fplan(pred=pred, pos=None) == INVALID and _fplan(pred=pred, count=None) == INVALID
    assert _fplan(pred=pred, pos=None, n=0) == INVALID and _fplan(pred=pred, count=None, n=0) == INVALID
    assert _fcount(pred=pred, count=None) == INVALID and _fcount(pred=pred, count=None, n=0) == INVALID
    assert _fwrite(pred=pred, ws=None) == INVALID
    if 'row' not in NEEDS[pred]:
        assert _fwrite(pred=pred, row=None) == INVALID                        # row_out wants row
    for n in (0, 5000, 2048 * 2048):
        need = L.tsamd_filter_workspace_bytes(i64(n))
        assert _fplan(pred=pred, n=n, ws=None) == WORKSPACE and _fplan(pred=pred, n=n, wsb=sz(need - 1)) == WORKSPACE
        need = L.tsamd_filter_tiles_workspace_bytes(i64(n))
        assert _fcount(pred=pred, n=n, ws=None) == WORKSPACE and _fcount(pred=pred, n=n, wsb=sz(need - 1)) == WORKSPACE
    assert _fwrite(pred=pred, n=0, row=None, col=None, mask=None, map=None, row_out=None, col_out=None, src_out=None) == OK


def test_status_filter_unknown_predicate_and_apply():
    for pred in (-1, 6):
        assert _fplan(pred=pred) == UNSUPPORTED and _fcount(pred=pred) == UNSUPPORTED and _fwrite(pred=pred) == UNSUPPORTED
        assert _fplan(pred=pred, n=0) == UNSUPPORTED and _fcount(pred=pred, n=0) == UNSUPPORTED
        assert _fwrite(pred=pred, n=0) == UNSUPPORTED
        assert _fplan(pred=pred, pos=None) == INVALID and _fcount(pred=pred, count=None) == INVALID   # NULL comes first
    assert _fapply(n=-1) == INVALID and _fapply(pos=None) == INVALID
    assert _fapply(row=None) == INVALID and _fapply(col=None) == INVALID
    assert _fapply(n=0, pos=None, row=None, col=None) == OK


def test_status_scatter_rows():
    def f(row=fake, col=fake, n=300, delta=fake, row_out=fake, col_out=fake, src_out=fake):
        return nat.lib().tsamd_scatter_rows(row, col, i64(n), delta, i64(0), i64(0), row_out, col_out, src_out, None)
    assert f(n=-1) == INVALID and f(row=None) == INVALID and f(delta=None) == INVALID and f(col=None) == INVALID
    assert f(n=0, row=None, col=None, delta=None) == OK


def test_status_diag():
    L = nat.lib()

    def mask(row=fake, col=fake, E=9, M=4, N=5, k=0, out=fake):
        return L.tsamd_non_diag_mask(row, col, i64(E), i64(M), i64(N), i64(k), out, None)

    def insert(row=fake, col=fake, E=9, M=4, N=5, k=0, row_out=fake, col_out=fake, src_out=fake):
        return L.tsamd_insert_diag(row, col, i64(E), i64(M), i64(N), i64(k), row_out, col_out, src_out, None)

    def apply(pos=fake, row=fake, col=fake, E=9, M=4, N=5, k=0, row_out=fake, col_out=fake, src_out=fake):
        return L.tsamd_set_diag_apply(pos, row, col, i64(E), i64(M), i64(N), i64(k), row_out, col_out, src_out, None)

    for f in (mask, insert, apply):
        assert f(E=-1) == INVALID and f(M=-1) == INVALID and f(N=-1) == INVALID
        assert f(row=None) == INVALID and f(col=None) == INVALID
    assert mask(out=None) == INVALID and mask(out=None, E=0) == INVALID       # (the diagonal alone has bytes)
    assert mask(out=None, row=None, col=None, E=0, k=9) == OK                 # no entry, no diagonal: nothing to write
    for f in (insert, apply):
        for name in ('row_out', 'col_out', 'src_out'):
            assert f(**{name: None}) == INVALID and f(**{name: None, 'E': 0}) == INVALID
    assert insert(E=0, k=9, row=None, col=None, row_out=None, col_out=None, src_out=None) == OK
    assert apply(pos=None) == INVALID and apply(pos=None, E=0, k=9) == INVALID
    assert apply(E=0, k=9, row=None, col=None, row_out=None, col_out=None, src_out=None) == OK
