"""The status ladders of the SpSpMM forward stages (csrc/spspmm.hip: tsamd_spspmm_plan / _symbolic / _numeric) pinned
with literal statuses.  Every call below returns before the first HIP call -- a refusal, or M == 0 -- so the dummy
pointers are never dereferenced and the file runs without a GPU.  The two stages do NOT test in the same order
(symbolic: range, M == 0, pointers, counts, dtype, workspace; numeric: dtype first): callers see that order through
the status they get for an argument tuple that is wrong twice, so it is part of the interface."""
import ctypes

import pytest

from pytorch_sparse_amd import _native as nat

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
F32, F64, F16 = 0, 1, 2
i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
FAKE = 0x1000  # never dereferenced

BASE = dict(dtype=F32, rowptrA=FAKE, colA=FAKE, valA=None, rowptrB=FAKE, colB=FAKE, valB=None, M=4, N=4, prod=FAKE,
            bins=FAKE, n_medium=0, n_large=0, P_large=0, out=FAKE, colC=FAKE, valC=None, flag=0, workspace=None,
            workspace_bytes=0)


def _p(x):
    return None if x is None else vp(x)


def symbolic(**kw):
    a = dict(BASE, **kw)
    return nat.lib().tsamd_spspmm_symbolic(
        a['dtype'], _p(a['rowptrA']), _p(a['colA']), _p(a['valA']), _p(a['rowptrB']), _p(a['colB']), _p(a['valB']),
        a['flag'], i64(a['M']), i64(a['N']), _p(a['prod']), _p(a['bins']), i64(a['n_medium']), i64(a['n_large']),
        i64(a['P_large']), _p(a['out']), _p(a['workspace']), sz(a['workspace_bytes']), None)


def numeric(**kw):
    a = dict(BASE, **kw)
    return nat.lib().tsamd_spspmm_numeric(
        a['dtype'], _p(a['rowptrA']), _p(a['colA']), _p(a['valA']), _p(a['rowptrB']), _p(a['colB']), _p(a['valB']),
        i64(a['M']), i64(a['N']), _p(a['prod']), _p(a['bins']), i64(a['n_medium']), i64(a['n_large']),
        i64(a['P_large']), _p(a['out']), _p(a['colC']), _p(a['valC']), a['flag'], _p(a['workspace']),
        sz(a['workspace_bytes']), None)


def plan(rowptrA=FAKE, colA=FAKE, rowptrB=FAKE, colB64=FAKE, nnzB=0, M=4, prod=FAKE, bins=FAKE, colB32=FAKE,
         stats=FAKE):
    return nat.lib().tsamd_spspmm_plan(_p(rowptrA), _p(colA), _p(rowptrB), _p(colB64), i64(nnzB), i64(M), _p(prod),
                                       _p(bins), _p(colB32), _p(stats), None)


def need(dtype, n_large, P_large, N):
    return int(nat.lib().tsamd_spspmm_workspace_bytes(dtype, i64(n_large), i64(P_large), i64(N)))


STAGES = pytest.mark.parametrize('stage', [symbolic, numeric], ids=['symbolic', 'numeric'])


@STAGES
def test_sizes_out_of_range_are_unsupported(stage):
    assert stage(M=-1) == UNSUPPORTED
    assert stage(N=-1) == UNSUPPORTED
    assert stage(N=(1 << 32) - 1) == UNSUPPORTED   # column ids must stay below the 2^32 - 1 sentinel
    assert stage(N=1 << 40) == UNSUPPORTED
    assert stage(M=1 << 31) == UNSUPPORTED          # one workgroup per row: the grid is 32-bit
    # ... and before anything else of an fp32 / fp64 call is looked at
    assert stage(M=1 << 31, rowptrA=None, out=None, n_medium=-1) == UNSUPPORTED
    assert stage(dtype=F64, N=(1 << 32) - 1, n_large=1) == UNSUPPORTED


@STAGES
def test_largest_sizes_pass_the_range_test(stage):
    # the next refusal of the ladder answers, not the range test
    assert stage(N=(1 << 32) - 2, out=None) == INVALID
    assert stage(M=(1 << 31) - 1, out=None) == INVALID
    assert stage(M=(1 << 31) - 1, N=(1 << 32) - 2, n_medium=-1) == INVALID


@STAGES
def test_empty_product_is_ok_without_any_pointer(stage):
    nothing = dict(rowptrA=None, colA=None, rowptrB=None, colB=None, prod=None, bins=None, out=None, colC=None)
    assert stage(M=0, **nothing) == OK
    assert stage(M=0, N=0, **nothing) == OK
    assert stage(dtype=F64, M=0, n_medium=5, n_large=-3, **nothing) == OK  # the counts are not looked at either
    assert stage(M=0, N=(1 << 32) - 1, **nothing) == UNSUPPORTED            # the range is


def test_dtype_comes_first_in_numeric_and_fifth_in_symbolic():
    assert symbolic(dtype=F16, M=0) == OK
    assert numeric(dtype=F16, M=0) == UNSUPPORTED
    assert symbolic(dtype=F16, rowptrA=None) == INVALID
    assert numeric(dtype=F16, rowptrA=None) == UNSUPPORTED
    assert symbolic(dtype=F16, n_medium=-1) == INVALID
    assert numeric(dtype=F16, n_medium=-1) == UNSUPPORTED
    for dtype in (F16, 3, 4, 5, 42, -1):
        assert symbolic(dtype=dtype) == UNSUPPORTED
        assert numeric(dtype=dtype) == UNSUPPORTED
    # symbolic: the dtype before the workspace
    assert symbolic(dtype=F16, n_large=1, P_large=9000) == UNSUPPORTED


@STAGES
@pytest.mark.parametrize('name', ['rowptrA', 'rowptrB', 'prod', 'bins', 'out'])
def test_null_pointers_are_invalid(stage, name):
    assert stage(**{name: None}) == INVALID
    assert stage(dtype=F64, n_medium=-1, **{name: None}) == INVALID
    assert stage(n_large=1, P_large=9000, **{name: None}) == INVALID  # before the workspace


@STAGES
def test_operands_without_entries_need_no_columns(stage):
    # colA / colB (and the values) may be NULL: the ladder goes on to the next line
    assert stage(colA=None, colB=None, n_large=1, P_large=9000) == WORKSPACE
    assert stage(colA=None, colB=None, n_medium=-1) == INVALID


def test_numeric_does_not_ask_for_colC():
    assert numeric(colC=None, valC=None, n_large=1, P_large=9000) == WORKSPACE


@STAGES
def test_counts(stage):
    assert stage(n_medium=-1) == INVALID
    assert stage(n_large=-1) == INVALID
    assert stage(M=4, n_medium=3, n_large=2) == INVALID                               # M + 1
    assert stage(M=4, n_medium=0, n_large=5, P_large=9000) == INVALID                  # before the workspace
    assert stage(M=4, n_medium=3, n_large=1, P_large=9000) == WORKSPACE                # == M passes
    assert stage(dtype=F64, M=4, n_medium=0, n_large=4, P_large=9000) == WORKSPACE
    assert symbolic(dtype=F16, M=4, n_medium=4, n_large=0) == UNSUPPORTED             # == M passes, then the dtype


@STAGES
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('N', [4, 500000, (1 << 24) + 1, 1 << 27])
def test_workspace(stage, dtype, N):
    n = need(dtype, 3, 9000, N)
    assert n > 0
    assert stage(dtype=dtype, M=8, N=N, n_large=3, P_large=9000, workspace=None, workspace_bytes=n) == WORKSPACE
    assert stage(dtype=dtype, M=8, N=N, n_large=3, P_large=9000, workspace=FAKE, workspace_bytes=0) == WORKSPACE
    assert stage(dtype=dtype, M=8, N=N, n_large=3, P_large=9000, workspace=FAKE, workspace_bytes=n - 1) == WORKSPACE


def test_workspace_bytes():
    for dtype in (F32, F64, F16):
        for n_large in (0, -1, -(1 << 40)):
            assert need(dtype, n_large, 9000, 500000) == 0
            assert need(dtype, n_large, 0, (1 << 32) - 2) == 0
    # every piece is a multiple of 256 bytes; fp64 keeps 4 + 8 bytes per product where fp32 keeps one 8-byte pair
    for dtype in (F32, F64):
        a, b = need(dtype, 3, 9000, 500000), need(dtype, 3, 9000 + 6400, 500000)
        assert a % 256 == 0 and a > 0
        assert b - a == 6400 * (8 if dtype == F32 else 12)
    assert need(F16, 3, 9000, 500000) == need(F32, 3, 9000, 500000)  # (anything but fp64 is sized as 4 bytes)


def test_plan_refuses_before_the_first_launch():
    assert plan(M=-1) == INVALID
    assert plan(stats=None) == INVALID
    assert plan(nnzB=-1) == INVALID
    assert plan(nnzB=5, colB64=None) == INVALID
    assert plan(nnzB=5, colB32=None) == INVALID
    assert plan(M=0, stats=None, nnzB=0, colB64=None, colB32=None) == INVALID
    # B without entries: nothing is narrowed, so the operands of M > 0 rows are looked at before any HIP call
    for name in ('rowptrA', 'rowptrB', 'bins', 'prod'):
        assert plan(nnzB=0, colB64=None, colB32=None, **{name: None}) == INVALID
