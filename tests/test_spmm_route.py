"""What the SpMM forward (csrc/spmm_kernels.h) decides before it launches, pinned through tsamd_spmm_route at every
threshold and its neighbours, and the status code for every argument it refuses -- host arithmetic only, runs without
a GPU.  Every row comes from a comment or a constant of spmm_kernels.h, named beside it; the expected values are
literals on purpose: a planner that silently takes another route still computes the right product and only the
time -- or the coverage of tests/test_spmm_forward_routes_gpu.py -- changes, so whoever moves TSAMD_TARGET_WAVES, the
items caps, relabel_possible, kHotBlockMinN or the packet ladder has to revisit this table knowingly.

Pointers are plain addresses here: the query uses them for their alignment and their distances only."""
import ctypes

import pytest
import torch

from pytorch_sparse_amd import _native as nat

F32, F64, F16, BF16, I32, I64, U8 = (torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32,
                                     torch.int64, torch.uint8)
A = 1 << 30    # an aligned operand address
WS = 1 << 32   # a workspace address (256-byte aligned)
W = 32768      # TSAMD_TARGET_WAVES


def route(dtype, reduce, B, M, N, K, E, **kw):
    kw.setdefault('mat', A)
    kw.setdefault('out', 2 * A)
    kw.setdefault('arg_out', 3 * A)
    kw.setdefault('workspace', WS)
    return nat.spmm_route(dtype, reduce, B, M, N, K, E, **kw)


def status(dtype_code, reduce_code, B, M, N, K, E, arg32=0, workspace=WS, null_route=False):
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    out = (ctypes.c_int64 * 24)()
    return nat.lib().tsamd_spmm_route(dtype_code, reduce_code, i64(B), i64(M), i64(N), i64(K), i64(E), vp(A), vp(2 * A),
                                      vp(3 * A), arg32, vp(workspace), None if null_route else out)


# plan_partition: items = clamp(ceil((M + E) / 32768), 128, cap); cap 1024 for rows <= 128 B (kShortRowItems), 256 for
# <= 512 B, 512 for < 1024 B, 1024 above.  (dtype, K, M + E) -> items
ITEMS = [
    (F32, 64, 1, 128), (F32, 64, 128 * W, 128), (F32, 64, 128 * W + 1, 129), (F32, 64, 200 * W, 200),
    (F32, 64, 255 * W + 1, 256), (F32, 64, 256 * W, 256), (F32, 64, 256 * W + 1, 256), (F32, 64, 2000 * W, 256),
    (F32, 128, 2000 * W, 256),                                  # 512 B: still the 256 class
    (F32, 129, 2000 * W, 512), (F32, 132, 300 * W, 300), (F32, 132, 512 * W, 512), (F32, 132, 512 * W + 1, 512),
    (F32, 255, 2000 * W, 512), (BF16, 260, 2000 * W, 512), (BF16, 511, 2000 * W, 512),
    (F32, 256, 2000 * W, 1024), (F32, 256, 1024 * W, 1024), (F32, 256, 1000 * W, 1000), (BF16, 512, 2000 * W, 1024),
    (F32, 32, 2000 * W, 1024), (F32, 32, 600 * W, 600), (BF16, 64, 2000 * W, 1024), (F32, 33, 2000 * W, 256),
    (F64, 16, 2000 * W, 1024), (F64, 17, 2000 * W, 256),
]


@pytest.mark.parametrize('dtype,K,total,items', ITEMS)
def test_items_and_partitions(dtype, K, total, items):
    M = min(4096, total)
    r = route(dtype, 'sum', 1, M, 64, K, total - M)
    assert r['items'] == items and r['P'] == -(-total // items)
    assert r['fixup'] == (1 if r['P'] > 1 else 0) and r['snap'] == 0
    # min / max snap to row starts: TSAMD_RECORD_SNAP = 128, items / 2 at most
    assert route(dtype, 'max', 1, M, 64, K, total - M)['snap'] == min(128, items // 2)


def test_one_partition_has_no_fixup():
    assert route(F32, 'sum', 1, 28, 64, 64, 100)['P'] == 1 and route(F32, 'sum', 1, 28, 64, 64, 100)['fixup'] == 0
    r = route(F32, 'sum', 1, 28, 64, 64, 101)
    assert (r['P'], r['fixup']) == (2, 1)


E20 = 1 << 20
# relabel_possible: E >= 2^20, N >= 4096, E >= 8 N, rows a multiple of 16 B, a power of two >= 256 B; min / max only for
# 4- and 8-byte types.  Hot rows: sums / means, B == 1; hot blocks from N = kHotBlockMinN = 65536.
# (dtype, reduce, B, N, K, E, mat offset) -> relabel, copy, family
COPY = [
    (F32, 'sum', 2, 4096, 64, E20, 0, 2, 1, 'cooperative'),       # B > 1 leaves the hot scope: the full copy
    (F32, 'sum', 2, 4096, 64, E20 - 1, 0, 0, 0, 'cooperative'),
    (F32, 'sum', 2, 4095, 64, E20, 0, 0, 0, 'cooperative'),
    (F32, 'sum', 2, 131072, 64, E20, 0, 2, 1, 'cooperative'),     # E == 8 N
    (F32, 'sum', 2, 131073, 64, E20, 0, 0, 0, 'cooperative'),
    (F32, 'sum', 2, 4096, 32, E20, 0, 0, 0, 'short'),             # 128-byte rows
    (F32, 'sum', 2, 4096, 96, E20, 0, 0, 0, 'cooperative'),       # 384 B: no power of two
    (F32, 'sum', 2, 4096, 128, E20, 0, 2, 1, 'cooperative'),
    (F32, 'sum', 2, 4096, 66, E20, 0, 0, 0, 'cooperative'),       # 264 B: no multiple of 16
    (BF16, 'sum', 2, 4096, 128, E20, 0, 2, 1, 'cooperative'),
    (BF16, 'max', 1, 4096, 128, E20, 0, 0, 0, 'cooperative'),     # min / max of 2-byte types never copy
    (F16, 'min', 1, 4096, 256, E20, 0, 0, 0, 'cooperative'),
    (F32, 'max', 1, 4096, 64, E20, 0, 2, 1, 'cooperative'),       # fp32 / fp64 min / max: the full copy
    (F64, 'min', 1, 4096, 32, E20, 0, 2, 1, 'cooperative'),
    (F32, 'max', 1, 4096, 32, E20, 0, 0, 0, 'short'),
    (F32, 'sum', 1, 4096, 64, E20, 0, 2, 2, 'hot_rows'),
    (F32, 'mean', 1, 4096, 64, E20, 0, 2, 2, 'hot_rows'),
    (F64, 'sum', 1, 4096, 32, E20, 0, 2, 2, 'hot_rows'),
    (BF16, 'sum', 1, 4096, 128, E20, 0, 2, 2, 'hot_rows'),
    (F32, 'sum', 1, 65535, 64, E20, 0, 2, 2, 'hot_rows'),
    (F32, 'sum', 1, 65536, 64, E20, 0, 2, 3, 'hot_blocks'),
    (F32, 'sum', 2, 65536, 64, E20, 0, 2, 1, 'cooperative'),
    (I32, 'sum', 1, 4096, 64, E20, 0, 2, 1, 'cooperative'),       # integer sums copy, the table is floating point only
    (F32, 'sum', 1, 4096, 64, E20, 16, 2, 2, 'hot_rows'),         # mat 16 bytes into its storage: still hot
    (F32, 'sum', 1, 4096, 64, E20, 8, 2, 1, 'cooperative'),       # 8 bytes: vec 2, the table needs 16 -> full copy
    (F32, 'sum', 1, 4096, 64, E20, 4, 0, 0, 'cooperative'),       # 4 bytes: single elements, no copy at all (VEC > 1)
    (F64, 'sum', 1, 4096, 32, E20, 8, 0, 0, 'cooperative'),
    (F64, 'max', 1, 4096, 32, E20, 8, 0, 0, 'cooperative'),
]


@pytest.mark.parametrize('dtype,reduce,B,N,K,E,off,relabel,copy,family', COPY)
def test_relabel_and_hot_scope(dtype, reduce, B, N, K, E, off, relabel, copy, family):
    r = route(dtype, reduce, B, 2048, N, K, E, mat=A + off)
    assert (r['relabel'], r['copy'], r['family']) == (relabel, copy, family)


# packet ladder by K (kMaxVec: 4 elements for 1- and 2-byte types, 16 bytes otherwise) and the lane layout:
# slots = ceil(K / vec), lpr = the power of two >= slots (64 at most), lgG = 6 - log2(lpr), ktiles = ceil(slots / 64);
# lgG >= 3 is the short-row kernel.  (dtype, K) -> vec, slots, lpr, lgG, ktiles
LANES = [
    (F32, 4, 4, 1, 1, 6, 1), (F32, 8, 4, 2, 2, 5, 1), (F32, 12, 4, 3, 4, 4, 1), (F32, 16, 4, 4, 4, 4, 1),
    (F32, 20, 4, 5, 8, 3, 1), (F32, 32, 4, 8, 8, 3, 1), (F32, 36, 4, 9, 16, 2, 1), (F32, 64, 4, 16, 16, 2, 1),
    (F32, 68, 4, 17, 32, 1, 1), (F32, 128, 4, 32, 32, 1, 1), (F32, 132, 4, 33, 64, 0, 1), (F32, 256, 4, 64, 64, 0, 1),
    (F32, 260, 4, 65, 64, 0, 2), (F32, 520, 4, 130, 64, 0, 3), (F32, 66, 2, 33, 64, 0, 1), (F32, 65, 1, 65, 64, 0, 2),
    (F32, 3, 1, 3, 4, 4, 1), (F32, 1, 1, 1, 1, 6, 1), (F32, 602, 2, 301, 64, 0, 5),
    (BF16, 64, 4, 16, 16, 2, 1), (BF16, 66, 2, 33, 64, 0, 1), (BF16, 65, 1, 65, 64, 0, 2), (F16, 8, 4, 2, 2, 5, 1),
    (F64, 64, 2, 32, 32, 1, 1), (F64, 65, 1, 65, 64, 0, 2), (F64, 16, 2, 8, 8, 3, 1),
    (I64, 6, 2, 3, 4, 4, 1), (I32, 6, 2, 3, 4, 4, 1), (I32, 8, 4, 2, 2, 5, 1), (U8, 8, 4, 2, 2, 5, 1), (U8, 6, 2, 3, 4, 4, 1),
]


@pytest.mark.parametrize('dtype,K,vec,slots,lpr,lgG,ktiles', LANES)
def test_packet_width_by_k_and_lane_layout(dtype, K, vec, slots, lpr, lgG, ktiles):
    for B in (1, 3):
        r = route(dtype, 'sum', B, 1000, 500, K, 20000)
        assert (r['vec'], r['slots'], r['lpr'], r['lgG'], r['ktiles']) == (vec, slots, lpr, lgG, ktiles)
        assert r['family'] == ('short' if lgG >= 3 else 'cooperative') and r['grid_y'] == B * ktiles


# packet ladder by pointer: mat / out aligned to vec * element size, arg_out to vec * 8 bytes, vec * 4 with arg32
# (dtype, reduce, arg32, which pointer, offset in bytes) -> vec
POINTERS = [
    (F32, 'sum', 0, 'mat', 16, 4), (F32, 'sum', 0, 'mat', 8, 2), (F32, 'sum', 0, 'mat', 4, 1), (F32, 'sum', 0, 'mat', 12, 1),
    (F32, 'sum', 0, 'out', 8, 2), (F32, 'sum', 0, 'out', 4, 1), (F32, 'sum', 0, 'arg_out', 4, 4),  # sums have no ids
    (F32, 'max', 0, 'mat', 8, 2), (F32, 'max', 0, 'out', 4, 1),
    (F32, 'max', 0, 'arg_out', 32, 4), (F32, 'max', 0, 'arg_out', 16, 2), (F32, 'max', 0, 'arg_out', 8, 1),
    (F32, 'max', 1, 'arg_out', 16, 4), (F32, 'max', 1, 'arg_out', 8, 2), (F32, 'max', 1, 'arg_out', 4, 1),
    (BF16, 'sum', 0, 'mat', 8, 4), (BF16, 'sum', 0, 'mat', 4, 2), (BF16, 'sum', 0, 'mat', 2, 1), (BF16, 'sum', 0, 'out', 4, 2),
    (BF16, 'min', 0, 'arg_out', 32, 4), (BF16, 'min', 0, 'arg_out', 16, 2), (BF16, 'min', 0, 'arg_out', 8, 1),
    (BF16, 'min', 1, 'arg_out', 16, 4), (BF16, 'min', 1, 'arg_out', 8, 2), (BF16, 'min', 1, 'arg_out', 4, 1),
    (F64, 'sum', 0, 'mat', 8, 1), (F64, 'max', 0, 'arg_out', 8, 1), (F64, 'max', 1, 'arg_out', 4, 1), (F64, 'max', 1, 'arg_out', 8, 2),
    (I64, 'max', 0, 'out', 8, 1), (U8, 'sum', 0, 'mat', 2, 2), (U8, 'sum', 0, 'mat', 1, 1),
]


@pytest.mark.parametrize('dtype,reduce,arg32,which,off,vec', POINTERS)
def test_packet_width_by_pointer(dtype, reduce, arg32, which, off, vec):
    base = {'mat': A, 'out': 2 * A, 'arg_out': 3 * A}
    base[which] += off
    assert route(dtype, reduce, 1, 1000, 500, 64, 20000, arg32=bool(arg32), **base)['vec'] == vec


def test_all_three_pointers_off_by_one_element():
    assert route(F32, 'max', 1, 1000, 500, 64, 20000, mat=A + 4, out=2 * A + 4, arg_out=3 * A + 8)['vec'] == 1
    assert route(F32, 'max', 1, 1000, 500, 64, 20000, mat=A + 8, out=2 * A + 8, arg_out=3 * A + 16)['vec'] == 2
    assert route(F32, 'max', 1, 1000, 500, 64, 20000, mat=0, out=0, arg_out=0)['vec'] == 4  # NULL means aligned


# int32 ids: their own instantiations, and the record-writing forward's window (spmm_emits_records: fp32 / f16 / bf16,
# 33..256 features in four-element packets, fp32 only above 64; 32-byte records for 97..128 features)
RECORDS = [
    (F32, 32, 'arg32_short', 0), (F32, 36, 'arg32_cooperative', 0), (F32, 64, 'arg32_cooperative', 0),
    (F32, 68, 'arg32_cooperative', 2), (F32, 96, 'arg32_cooperative', 2), (F32, 100, 'arg32_cooperative', 1),
    (F32, 128, 'arg32_cooperative', 1), (F32, 132, 'arg32_cooperative', 2), (F32, 256, 'arg32_cooperative', 2),
    (F32, 260, 'arg32_cooperative', 0), (F32, 98, 'arg32_cooperative', 0),
    (BF16, 32, 'arg32_short', 0), (BF16, 36, 'arg32_cooperative', 2), (BF16, 64, 'arg32_cooperative', 2),
    (F16, 128, 'arg32_cooperative', 1), (BF16, 256, 'arg32_cooperative', 2), (BF16, 260, 'arg32_cooperative', 0),
    (F64, 64, 'arg32_cooperative', 0), (F64, 16, 'arg32_short', 0),
]


@pytest.mark.parametrize('dtype,K,family,records', RECORDS)
def test_arg32_family_and_records_window(dtype, K, family, records):
    r = route(dtype, 'max', 1, 1000, 500, K, 20000, arg32=True)
    assert (r['family'], r['records']) == (family, records)
    i64 = ctypes.c_int64
    says = nat.lib().tsamd_spmm_minmax_records_in_forward(nat.dtype_code(dtype), i64(1), i64(1000), i64(K), i64(20000))
    assert says == (1 if records else 0)
    assert route(dtype, 'max', 1, 1000, 500, K, 20000)['records'] == 0  # int64 ids never write records
    if records:  # the record writer's lane layout assumes four-element packets
        assert route(dtype, 'max', 1, 1000, 500, K, 20000, arg32=True, mat=A + 4)['records'] == 0


def test_offsets_and_workspace_bytes():
    i64 = ctypes.c_int64
    for dtype, reduce, B, M, N, K, E in [(F32, 'sum', 1, 1000, 500, 64, 20000), (BF16, 'max', 3, 77, 500, 260, 90000),
                                         (F32, 'sum', 1, 2048, 4096, 64, E20), (F64, 'min', 2, 2048, 4096, 32, E20)]:
        r = route(dtype, reduce, B, M, N, K, E)
        P = r['P']
        pad = lambda n: -(-n // 256) * 256  # noqa: E731
        acc = 8 if dtype == F64 else 4
        minmax = reduce in ('min', 'max')
        assert r['table_off'] == 0 and r['tail_row_off'] == pad(16 * (P + 1))
        flag = r['tail_row_off'] + pad(8 * P) + 2 * pad(acc * B * P * K) + (2 * pad(4 * B * P * K) if minmax else 0)
        assert r['relabel_flag_off'] == flag
        assert r['head_row_off'] >= flag + 256 and r['head_row_off'] + 8 * P <= r['workspace_bytes']
        assert r['workspace_bytes'] == nat.lib().tsamd_spmm_workspace_bytes(
            nat.dtype_code(dtype), nat.REDUCES[reduce], i64(B), i64(M), i64(N), i64(K), i64(E))
        r0 = route(dtype, reduce, B, M, N, K, E, workspace=0)  # no workspace: the same decisions, offsets 0
        for k in ('table_off', 'tail_row_off', 'head_row_off', 'relabel_flag_off'):
            assert r0[k] == 0
            r0[k] = r[k]
        assert r0 == r


def test_status_codes():
    f32, s, mx = 0, 0, 3
    ok = (1, 100, 100, 64, 1000)
    assert status(f32, s, *ok) == 0
    for i in range(5):  # a negative size
        bad = list(ok)
        bad[i] = -1
        assert status(f32, s, *bad) == 1
    assert status(f32, s, *ok, null_route=True) == 1
    assert status(99, s, *ok) == 2 and status(f32, 4, *ok) == 2 and status(f32, -1, *ok) == 2
    assert status(f32, s, 1, 100, 1 << 32, 64, 1000) == 2 and status(f32, s, 1, 100, (1 << 32) - 1, 64, 1000) == 0
    assert status(f32, s, 1, 100, 100, 1 << 31, 1000) == 2
    assert status(f32, s, 65536, 100, 100, 1, 1000) == 2
    assert status(f32, s, 1024, 100, 100, 4096, 1000) == 2 and status(f32, s, 1023, 100, 100, 4096, 1000) == 0
    assert status(f32, s, *ok, arg32=1) == 2            # int32 ids: min / max only ...
    assert status(4, mx, *ok, arg32=1) == 2             # ... of the floating types ...
    assert status(f32, mx, 1, 100, 100, 64, 1 << 31, arg32=1) == 2  # ... and E itself must fit
    assert status(f32, mx, 1, 100, 100, 64, (1 << 31) - 1, arg32=1) == 0
    assert status(f32, s, *ok, workspace=WS + 128) == 4
    for empty in [(0, 100, 100, 64, 1000), (1, 0, 100, 64, 0), (1, 100, 100, 0, 1000)]:
        assert route(F32, 'sum', *empty) == dict(zip(nat.SPMM_ROUTE_FIELDS, ['none'] + [0] * 18))


def test_reference_order_reports_its_own_family():
    L = nat.lib()
    was = L.tsamd_spmm_reference_order(-1)
    try:
        L.tsamd_spmm_reference_order(1)
        assert route(F32, 'sum', 1, 1000, 500, 64, 20000) == dict(zip(nat.SPMM_ROUTE_FIELDS, ['reference_order'] + [0] * 18))
    finally:
        L.tsamd_spmm_reference_order(was)
    assert route(F32, 'sum', 1, 1000, 500, 64, 20000)['family'] == 'cooperative'


# the masked sum (the pull of the min / max backward) launches the cooperative masked kernel at every width: the family
# word says what is launched, whatever lgG.  K -> lgG of the sum
MASKED = [(8, 5), (16, 4), (32, 3), (64, 2)]


@pytest.mark.parametrize('K,lgG', MASKED)
def test_masked_sum_family_is_cooperative(K, lgG):
    r = nat.spmm_minmax_bw_route('ids64', F32, 1, 1000, 1000, K, 20000, False, True)
    assert (r['mat'], r['family'], r['sum_lgG']) == ('pull', 'cooperative', lgG)


def test_one_plan_behind_every_query():
    """tsamd_spmm_route, tsamd_spmm_hot_rows_layout, tsamd_spmm_hot_blocks_layout and tsamd_spmm_order_layout answer from
    one plan: over dtype x reduce x B x N x row bytes x E x mat offset x out offset (5760 calls, M = 2048) they agree."""
    import itertools
    L, i64, vp = nat.lib(), ctypes.c_int64, ctypes.c_void_p
    lay, order = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 8)()
    cases = 0
    for dtype, reduce, B, N, row_bytes, E, moff, ooff in itertools.product(
            (F32, F64, BF16, I32), ('sum', 'mean', 'max'), (1, 2), (4095, 4096, 65535, 65536, 131072), (128, 256, 384, 512),
            (1 << 20, 1 << 24), (0, 8, 16), (0, 8)):
        K = row_bytes // torch.empty(0, dtype=dtype).element_size()
        r = route(dtype, reduce, B, 2048, N, K, E, mat=A + moff, out=2 * A + ooff)
        args = (nat.dtype_code(dtype), nat.REDUCES[reduce], i64(B), i64(2048), i64(N), i64(K), i64(E), vp(A + moff),
                vp(2 * A + ooff), vp(WS))
        assert L.tsamd_spmm_hot_rows_layout(*args, lay) == (1 if r['copy'] == 2 else 0)
        assert L.tsamd_spmm_hot_blocks_layout(*args, lay) == (1 if r['copy'] == 3 else 0)
        if L.tsamd_spmm_order_layout(*args, order) != 0:
            assert reduce in ('sum', 'mean') and r['family'] in ('cooperative', 'hot_rows', 'hot_blocks')
        if r['copy'] == 3:
            assert nat.spmm_hints_bytes(dtype, reduce, B, 2048, N, K, E) > 0
        cases += 1
    assert cases == 5760


def test_build_flags_stay_zero():
    assert nat.lib().tsamd_build_flags() == 0
