"""Status codes and workspace sizes of the pull-formulated min / max backward (tsamd_spmm_minmax_bw_csc, _arg32 and
_records, include/tsamd.h), pinned as literals: what these entries answer BEFORE they touch the device is part of the
C-ABI, and the torch glue picks its route from it.  Fake non-null pointers; every call below fails or finishes before any
HIP call (each row says why), so this runs without a GPU.  The one host-side outcome that is left out is the int64-id
route with grad_value wanted and the masked SDDMM's conditions not met: it starts with a memset on the device."""
import ctypes

import pytest

from pytorch_sparse_amd import _native as nat

i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
F32, F64, F16, BF16, I32 = 0, 1, 2, 3, 4
P = 0x1000           # a 256-byte aligned "pointer": never dereferenced
ODD = 0x1008         # 8 modulo 16
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4


def _call(entry, dtype=BF16, rowptr=P, col=P, value=P, mat=P, grad_out=P, winners=P, colptr=P, csr2csc=P, row=P,
          grad_value=None, grad_mat=P, B=1, M=8, N=8, K=64, E=16, ws=None, ws_bytes=0):
    """entry: 'ids64' (tsamd_spmm_minmax_bw_csc), 'ids32' (_arg32) or 'records' (_records; `value` only says whether
    the matrix has values there)."""
    L = nat.lib()
    fn = {'ids64': L.tsamd_spmm_minmax_bw_csc, 'ids32': L.tsamd_spmm_minmax_bw_csc_arg32,
          'records': L.tsamd_spmm_minmax_bw_csc_records}[entry]
    third = ctypes.c_int(1 if value else 0) if entry == 'records' else vp(value)
    return fn(dtype, vp(rowptr), vp(col), third, vp(mat), vp(grad_out), vp(winners), vp(colptr), vp(csr2csc), vp(row),
              vp(grad_value), vp(grad_mat), i64(B), i64(M), i64(N), i64(K), i64(E), vp(ws), sz(ws_bytes), None)


ALL = ('ids64', 'ids32', 'records')
NARROW = ('ids32', 'records')  # the entries whose winners are 32-bit: ids, or records with 32-bit row ids

# (entries, keyword arguments, status) -- the comment says where the call ends
STATUS_CASES = [
    # a negative size is INVALID before anything is computed from the sizes
    (ALL, dict(M=-1), INVALID),
    (ALL, dict(B=-1), INVALID),
    (ALL, dict(E=-1), INVALID),
    # integer dtypes have no gradient: refused right after the sizes' signs
    (ALL, dict(dtype=I32), UNSUPPORTED),
    (ALL, dict(dtype=42), UNSUPPORTED),
    # 32-bit row / column / entry ids inside the kernels: the range check comes before any pointer is looked at
    (ALL, dict(N=1 << 32), UNSUPPORTED),
    (ALL, dict(M=1 << 32), UNSUPPORTED),
    (ALL, dict(E=1 << 32), UNSUPPORTED),
    (ALL, dict(K=1 << 31), UNSUPPORTED),
    # int32 ids (and records made from them) end at 2^31 entries: first check of the two 32-bit entries ...
    (NARROW, dict(E=1 << 31), UNSUPPORTED),
    # ... while the int64 entry goes on to ask for its workspace (no grad_value: nothing is launched before that)
    (('ids64', ), dict(E=1 << 31), WORKSPACE),
    # the records entry only exists for grad_mat (grad_value alone reads ids): its first check
    (('records', ), dict(grad_mat=None), UNSUPPORTED),
    (('records', ), dict(grad_mat=None, grad_value=P), UNSUPPORTED),
    # no records on a problem that has entries and outputs: its second check
    (('records', ), dict(winners=None), INVALID),
    # ... which comes before the 2^31 limit, and after the grad_mat one
    (('records', ), dict(winners=None, E=1 << 31), INVALID),
    (('records', ), dict(winners=None, grad_mat=None), UNSUPPORTED),
    # missing ids: the int32 entry looks at them before the dtype, the int64 entry after it
    (('ids64', 'ids32'), dict(winners=None), INVALID),
    (('ids32', ), dict(winners=None, dtype=I32), INVALID),
    (('ids64', ), dict(winners=None, dtype=I32), UNSUPPORTED),
    # an empty pattern needs no records, but a call without `mat` either is INVALID whatever its dtype
    (('records', ), dict(winners=None, E=0, mat=None, dtype=I32), INVALID),
    (('records', ), dict(winners=None, E=0, dtype=I32), UNSUPPORTED),
    # any other missing input of a non-empty problem
    (ALL, dict(rowptr=None), INVALID),
    (ALL, dict(col=None), INVALID),
    (ALL, dict(mat=None), INVALID),
    (ALL, dict(grad_out=None), INVALID),
    # grad_value from 32-bit winners exists only as the masked SDDMM beside grad_mat, which needs 16-byte packets:
    # bf16 K = 36 is 72 bytes a row -- UNSUPPORTED before the workspace is looked at (the caller widens the ids)
    (NARROW, dict(grad_value=P, K=36), UNSUPPORTED),
    # the same for a misaligned mat or grad_out at K = 64
    (NARROW, dict(grad_value=P, mat=ODD), UNSUPPORTED),
    (NARROW, dict(grad_value=P, grad_out=ODD), UNSUPPORTED),
    # and for grad_value alone (no grad_mat: the row-parallel kernel reads int64 ids); the records entry said so above
    (('ids32', ), dict(grad_value=P, grad_mat=None), UNSUPPORTED),
    # grad_mat needs the transposed pattern: checked before the route is chosen
    (ALL, dict(colptr=None), INVALID),
    (ALL, dict(csr2csc=None), INVALID),
    (ALL, dict(row=None), INVALID),
    (ALL, dict(colptr=None, grad_value=P), INVALID),
    # nothing asked for, or no column to write: OK without a launch (the records entry has refused the former above)
    (('ids64', 'ids32'), dict(grad_mat=None), OK),
    (ALL, dict(N=0), OK),
    (ALL, dict(N=0, winners=None, K=0), OK),
]


@pytest.mark.parametrize('entries,kwargs,want', STATUS_CASES)
def test_status_before_any_launch(entries, kwargs, want):
    for entry in entries:
        assert _call(entry, **kwargs) == want, (entry, kwargs)


def _ws_bytes(entry, dtype, B, M, N, K, E):
    L = nat.lib()
    fn = L.tsamd_spmm_minmax_bw_csc_records_workspace_bytes if entry == 'records' else L.tsamd_spmm_minmax_bw_csc_workspace_bytes
    return fn(dtype, i64(B), i64(M), i64(N), i64(K), i64(E))


@pytest.mark.parametrize('entry', ALL)
@pytest.mark.parametrize('grad_value', [None, P])  # not wanted / wanted and eligible for the masked SDDMM (128-byte rows, aligned)
def test_workspace_is_checked_before_the_first_launch(entry, grad_value):
    """With grad_value either not wanted or made by the masked SDDMM, the first thing launched is the record writer (or,
    on records, the SDDMM): the workspace check comes before it."""
    need = _ws_bytes(entry, BF16, 1, 8, 8, 64, 16)
    assert need > 0 and need % 256 == 0
    assert _call(entry, grad_value=grad_value, ws=None, ws_bytes=0) == WORKSPACE
    assert _call(entry, grad_value=grad_value, ws=None, ws_bytes=need) == WORKSPACE
    assert _call(entry, grad_value=grad_value, ws=P, ws_bytes=need - 1) == WORKSPACE
    assert _call(entry, grad_value=grad_value, ws=ODD, ws_bytes=need + 256) == WORKSPACE


# (dtype, B, M, N, K, E) -> (tsamd_spmm_minmax_bw_csc_workspace_bytes, tsamd_spmm_minmax_bw_csc_records_workspace_bytes)
WORKSPACE_BYTES = {
    (BF16, 1, 1000, 1000, 36, 20000): (693760, 53760),
    (BF16, 2, 1000, 1000, 36, 20000): (1381376, 101376),
    (BF16, 1, 1000, 1000, 128, 20000): (815104, 175104),
    (BF16, 2, 1000, 1000, 128, 20000): (1624064, 344064),
    (BF16, 1, 1000, 1000, 160, 20000): (857600, 217600),
    (BF16, 2, 1000, 1000, 160, 20000): (1708544, 428544),
    (BF16, 1, 1000, 1000, 260, 20000): (1309696, 349696),
    (BF16, 2, 1000, 1000, 260, 20000): (2612736, 692736),
    (BF16, 1, 1000, 1000, 128, 0): (9216, 9216),
    (F32, 1, 1000, 1200, 128, 20000): (816128, 176128),
    (F64, 2, 300, 300, 16, 5000): (183552, 23552),
}


def test_workspace_bytes_are_pinned():
    L = nat.lib()
    for shape, (csc, rec) in WORKSPACE_BYTES.items():
        assert _ws_bytes('ids64', *shape) == csc, shape
        assert _ws_bytes('records', *shape) == rec, shape
        dtype, B, M, N, K, E = shape
        # the int64 / int32 entries write the records into the front of their workspace
        assert csc == rec + L.tsamd_spmm_minmax_records_bytes(i64(B), i64(K), i64(E)), shape
    assert len(WORKSPACE_BYTES) >= 9
    for entry in ('ids64', 'records'):
        assert _ws_bytes(entry, 99, 1, 1000, 1000, 128, 20000) == 0   # unknown dtype
        assert _ws_bytes(entry, BF16, 1, 1000, -1, 128, 20000) == 0   # negative size
