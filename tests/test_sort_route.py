"""What the sort driver (csrc/sort.hip) decides from the sizes alone, pinned through tsamd_sort_route at every
threshold and its neighbours, and the status code of every sort entry point for every argument it refuses -- host
arithmetic and validation only, runs without a GPU.  The expected values are written out as literals on purpose: a
driver that silently takes another route (the one-sweep passes instead of the bucket path, pairs instead of packed
words) still sorts bit-exactly and only the time changes, so whoever moves kSmallSortMax, TSAMD_BK_MIN_ENTRIES,
TSAMD_BK_MAX_TOTAL_BITS, the tile sizes or the key layout has to revisit this table knowingly."""
import ctypes

import pytest

from pytorch_sparse_amd import _native as nat

FIELDS = ('route', 'key_bits', 'idx_bits', 'packed', 'passes', 'ride', 'tiles',
          'on', 'levels', 'strip', 'bits', 'bits1', 'kshift', 'shift', 'nb', 'cap')
i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t


def route(E, M, N, value_bytes=0, coalesce=0):
    out = (ctypes.c_int64 * 16)()
    st = nat.lib().tsamd_sort_route(i64(E), i64(M), i64(N), value_bytes, coalesce, out)
    assert st == 0, (E, M, N, value_bytes, coalesce, st)
    return tuple(int(x) for x in out)


OFF = (0, ) * 9   # no bucket plan
NONE = (0, ) * 11  # routes 0 and 1: no ride, no tiles, no plan

# (E, M, N, value_bytes, coalesce): route, key_bits, idx_bits, packed, passes, ride, tiles,
#                                   on, levels, strip, bits, bits1, kshift, shift, nb, cap
TABLE = [
    # the two rows to check by hand against layout_for / plan_buckets:
    # 19 + 19 key bits, 23 position bits, ceil(7.5 M / 8192) tiles; 2^bits >= 7.5 M / (0.954 * 0.8 * 8192) -> 11 bits
    ((7500000, 500000, 500000, 0, 0), (2, 38, 23, 1, 5, 0, 916, 1, 1, 0, 11, 11, 0, 50, 2048, 8192)),
    # 22 + 22 key bits, 27 position bits: pairs, ceil(75 M / 6144) tiles; 2^bits >= 75 M / (0.8 * 8192) -> 14 = 7 + 7
    ((75000000, 1 << 22, 1 << 22, 0, 0), (2, 44, 27, 0, 6, 0, 12208, 1, 2, 1, 14, 7, 30, 57, 16384, 8192)),
    # E at the thresholds, 18-bit keys (300 x 500): nothing / one launch / passes only / bucket plan
    ((0, 300, 500, 0, 0), (0, 18, 0, 1, 3) + NONE),
    ((1, 300, 500, 0, 0), (1, 18, 0, 0, 0) + NONE),
    ((2, 300, 500, 0, 0), (1, 18, 0, 0, 3) + NONE),
    ((1 << 13, 300, 500, 0, 0), (1, 18, 0, 0, 3) + NONE),
    (((1 << 13) + 1, 300, 500, 0, 0), (2, 18, 14, 1, 3, 0, 2) + OFF),
    (((1 << 17) - 1, 300, 500, 0, 0), (2, 18, 17, 1, 3, 0, 16) + OFF),
    ((1 << 17, 300, 500, 0, 0), (2, 18, 17, 1, 3, 0, 16, 1, 1, 0, 6, 6, 0, 29, 64, 8192)),
    # keys of 0 bits: the one-launch kernel copies, the general path takes the identity kernel
    ((5, 1, 1, 0, 0), (1, 0, 0, 0, 0) + NONE),
    ((1 << 13, 1, 1, 0, 0), (1, 0, 0, 0, 0) + NONE),
    (((1 << 13) + 1, 1, 1, 0, 0), (0, 0, 14, 1, 0) + NONE),
    ((200000, 1, 1, 0, 0), (0, 0, 18, 1, 0) + NONE),
    # 32-bit keys: the widest the one-launch sort takes
    ((1, 1 << 16, 1 << 16, 0, 0), (1, 32, 0, 0, 0) + NONE),
    ((5, 1 << 16, 1 << 16, 0, 0), (1, 32, 0, 0, 4) + NONE),
    ((1 << 13, 1 << 16, 1 << 16, 0, 0), (1, 32, 0, 0, 4) + NONE),
    (((1 << 13) + 1, 1 << 16, 1 << 16, 0, 0), (2, 32, 14, 1, 4, 0, 2) + OFF),
    ((200000, 1 << 16, 1 << 16, 0, 0), (2, 32, 18, 1, 4, 0, 25, 1, 1, 0, 5, 5, 0, 45, 32, 8192)),
    # 33-bit keys (M * N = 2^33, and M * N = 2^32 + 2^16 whose ids still take 16 + 17 bits): never one launch
    ((1, 1 << 17, 1 << 16, 0, 0), (0, 33, 0, 1, 5) + NONE),
    ((2, 1 << 17, 1 << 16, 0, 0), (2, 33, 1, 1, 5, 0, 1) + OFF),
    ((1 << 13, 1 << 17, 1 << 16, 0, 0), (2, 33, 13, 1, 5, 0, 1) + OFF),
    (((1 << 13) + 1, 1 << 17, 1 << 16, 0, 0), (2, 33, 14, 1, 5, 0, 2) + OFF),
    ((200000, 1 << 17, 1 << 16, 0, 0), (2, 33, 18, 1, 5, 0, 25, 1, 1, 0, 5, 5, 0, 46, 32, 8192)),
    ((1 << 13, 1 << 16, (1 << 16) + 1, 0, 0), (2, 33, 13, 1, 5, 0, 1) + OFF),
    # 63- and 64-bit keys: pairs once the position takes a second bit, no bucket plan (the tile bits do not fit)
    ((1, 1 << 32, 1 << 31, 0, 0), (0, 63, 0, 1, 8) + NONE),
    ((2, 1 << 32, 1 << 31, 0, 0), (2, 63, 1, 1, 8, 0, 1) + OFF),
    (((1 << 13) + 1, 1 << 32, 1 << 31, 0, 0), (2, 63, 14, 0, 8, 0, 2) + OFF),
    ((200000, 1 << 32, 1 << 31, 0, 0), (2, 63, 18, 0, 8, 0, 33) + OFF),
    ((200000, 1 << 32, 1 << 32, 0, 0), (2, 64, 18, 0, 8, 0, 33) + OFF),
    # key_bits + idx_bits = 64 | 65: packed words with a full-word plan | pairs with a strip plan; a 4-byte
    # value rides in packed words only
    ((1 << 20, 1 << 22, 1 << 22, 0, 0), (2, 44, 20, 1, 6, 0, 128, 1, 1, 0, 8, 8, 0, 56, 256, 8192)),
    (((1 << 20) + 1, 1 << 22, 1 << 22, 0, 0), (2, 44, 21, 0, 6, 0, 171, 1, 1, 1, 8, 8, 36, 57, 256, 8192)),
    ((1 << 20, 1 << 22, 1 << 22, 4, 0), (2, 44, 20, 1, 6, 1, 171, 1, 1, 0, 8, 8, 0, 56, 256, 6144)),
    (((1 << 20) + 1, 1 << 22, 1 << 22, 4, 0), (2, 44, 21, 0, 6, 0, 171, 1, 1, 1, 8, 8, 36, 57, 256, 6144)),
    # value_bytes x coalesce at 7.5 M entries: 4 bytes ride (12-byte entries: smaller tiles, smaller buckets), 8
    # bytes do not
    ((7500000, 500000, 500000, 0, 0), (2, 38, 23, 1, 5, 0, 916, 1, 1, 0, 11, 11, 0, 50, 2048, 8192)),
    ((7500000, 500000, 500000, 0, 1), (2, 38, 23, 1, 5, 0, 916, 1, 1, 0, 11, 11, 0, 50, 2048, 8192)),
    ((7500000, 500000, 500000, 4, 0), (2, 38, 23, 1, 5, 1, 1221, 1, 1, 0, 11, 11, 0, 50, 2048, 6144)),
    ((7500000, 500000, 500000, 4, 1), (2, 38, 23, 1, 5, 1, 1221, 1, 1, 0, 11, 11, 0, 50, 2048, 6144)),
    ((7500000, 500000, 500000, 8, 0), (2, 38, 23, 1, 5, 0, 916, 1, 1, 0, 11, 11, 0, 50, 2048, 8192)),
    ((7500000, 500000, 500000, 8, 1), (2, 38, 23, 1, 5, 0, 916, 1, 1, 0, 11, 11, 0, 50, 2048, 8192)),
    # a riding value needs two passes at least (8- | 9-bit keys)
    (((1 << 13) + 1, 16, 16, 4, 0), (2, 8, 14, 1, 1, 0, 2) + OFF),
    (((1 << 13) + 1, 10, 20, 4, 0), (2, 9, 14, 1, 2, 1, 2) + OFF),
    (((1 << 13) + 1, 300, 500, 8, 0), (2, 18, 14, 1, 3, 0, 2) + OFF),
    ((5000, 1 << 20, 1 << 20, 4, 1), (2, 40, 13, 1, 5, 1, 1) + OFF),
    # full-word plans whose bucket id reaches into the position bits (shift < idx_bits): dropped by a compacting
    # sort; shift == idx_bits stays
    ((900000, 3, 5, 0, 0), (2, 5, 20, 1, 1, 0, 110, 1, 1, 0, 8, 8, 0, 17, 256, 8192)),
    ((900000, 3, 5, 0, 1), (2, 5, 20, 1, 1, 0, 110) + OFF),
    ((1 << 20, 16, 16, 0, 0), (2, 8, 20, 1, 1, 0, 128, 1, 1, 0, 8, 8, 0, 20, 256, 8192)),
    ((1 << 20, 16, 16, 0, 1), (2, 8, 20, 1, 1, 0, 128, 1, 1, 0, 8, 8, 0, 20, 256, 8192)),
    ((1 << 20, 16, 16, 4, 1), (2, 8, 20, 1, 1, 0, 128, 1, 1, 0, 8, 8, 0, 20, 256, 6144)),
    # strip plans: 11 bits are the last single level, 12 the first with two (6 + 6)
    ((3000000, 2097157, 2097149, 0, 0), (2, 43, 22, 0, 6, 0, 489, 1, 1, 1, 10, 10, 33, 55, 1024, 8192)),
    ((12500000, 1 << 21, 1 << 21, 0, 0), (2, 42, 24, 0, 6, 0, 2035, 1, 1, 1, 11, 11, 31, 55, 2048, 8192)),
    ((12500000, 1 << 21, 1 << 21, 4, 0), (2, 42, 24, 0, 6, 0, 2035, 1, 2, 1, 12, 6, 30, 54, 4096, 6144)),
    ((13421772, 1 << 21, 1 << 21, 0, 0), (2, 42, 24, 0, 6, 0, 2185, 1, 1, 1, 11, 11, 31, 55, 2048, 8192)),
    ((13421773, 1 << 21, 1 << 21, 0, 0), (2, 42, 24, 0, 6, 0, 2185, 1, 2, 1, 12, 6, 30, 54, 4096, 8192)),
    # kBkMaxTotalBits = 14: the last E it covers at 80 % fill, the first it does not; keys too wide for two
    # levels (45 - 7 + 27 > 64)
    ((75000000, 1 << 22, 1 << 22, 4, 1), (2, 44, 27, 0, 6, 0, 12208, 1, 2, 1, 14, 7, 30, 57, 16384, 6144)),
    ((107374182, 1 << 22, 1 << 22, 0, 0), (2, 44, 27, 0, 6, 0, 17477, 1, 2, 1, 14, 7, 30, 57, 16384, 8192)),
    ((107374183, 1 << 22, 1 << 22, 0, 0), (2, 44, 27, 0, 6, 0, 17477) + OFF),
    ((75000000, 1 << 23, 1 << 22, 0, 0), (2, 45, 27, 0, 6, 0, 12208) + OFF),
    ((75000000, 1 << 23, 1 << 23, 0, 0), (2, 46, 27, 0, 6, 0, 12208) + OFF),
]


@pytest.mark.parametrize('case', range(len(TABLE)))
def test_route_table(case):
    args, want = TABLE[case]
    assert dict(zip(FIELDS, route(*args))) == dict(zip(FIELDS, want)), args


def test_route_refuses_what_the_sorts_refuse():
    L = nat.lib()
    out = (ctypes.c_int64 * 16)()
    for E, M, N in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        assert L.tsamd_sort_route(i64(E), i64(M), i64(N), 0, 0, out) == 1
    for vb in (-4, 1, 2, 16):
        assert L.tsamd_sort_route(i64(4), i64(4), i64(4), vb, 0, out) == 1
    assert L.tsamd_sort_route(i64(4), i64(4), i64(4), 0, 0, None) == 1
    assert L.tsamd_sort_route(i64(5), i64(1 << 40), i64(1 << 40), 0, 0, out) == 2   # 80 key bits
    assert L.tsamd_sort_route(i64(5), i64(1 << 33), i64(1 << 32), 0, 0, out) == 2   # 65
    assert L.tsamd_sort_route(i64(5), i64(1 << 32), i64(1 << 32), 0, 0, out) == 0   # 64: the widest key
    assert L.tsamd_sort_route(i64(1 << 32), i64(4), i64(4), 0, 0, out) == 2         # positions are 32-bit
    assert L.tsamd_sort_route(i64((1 << 32) - 1), i64(4), i64(4), 0, 0, out) == 0


def test_sort_header_location():
    """tsamd_sort_header: the header opens the sort's own workspace; in the workspace of tsamd_sort_coalesce* the
    2^14 status words of the compacting bucket sort and the compaction kernel's state (8 + ceil(E / 2048) words, rounded
    up to 256 bytes) lie in front of it.  Words: #descents 0, fast 5, error 2."""
    L = nat.lib()
    out = (ctypes.c_int64 * 4)()
    for E, pre in ((0, 131072 + 256), (1, 131072 + 256), (9000, 131072 + 256), (1 << 17, 131072 + 768),
                   ((1 << 20) + 1, 131072 + 4352), (7500000, 131072 + 29440)):
        assert L.tsamd_sort_header(i64(E), 0, out) == 0 and list(out) == [0, 0, 5, 2], E
        assert L.tsamd_sort_header(i64(E), 1, out) == 0 and list(out) == [pre, 0, 5, 2], E
        assert pre + L.tsamd_sort_coo_workspace_bytes(i64(E)) == L.tsamd_sort_coalesce_workspace_bytes(i64(E))
    assert L.tsamd_sort_header(i64(-1), 0, out) == 1 and L.tsamd_sort_header(i64(5), 0, None) == 1


# ---- status codes: every case fails (or finishes) before any HIP call; `fake` is never dereferenced ----
fake = vp(0x1000)
BIG = sz(1 << 40)
I = dict(E=9000, M=300, N=500)  # noqa: E741  (above the one-launch sort)


def _sort_coo(row=fake, col=fake, E=9000, M=300, N=500, perm=fake, ws=fake, wsb=BIG):
    return nat.lib().tsamd_sort_coo(row, col, i64(E), i64(M), i64(N), fake, fake, perm, ws, wsb, None)


def _auto(name, row=fake, col=fake, E=9000, M=300, N=500, perm=fake, counts=fake, ws=fake, wsb=BIG):
    return getattr(nat.lib(), name)(row, col, i64(E), i64(M), i64(N), fake, fake, perm, counts, ws, wsb, None)


def _values(mode=0, row=fake, col=fake, E=9000, M=300, N=500, perm=fake, counts=fake, value=None, value_out=None,
            value_bytes=0, ws=fake, wsb=BIG):
    return nat.lib().tsamd_sort_coo_values(mode, row, col, i64(E), i64(M), i64(N), fake, fake, perm, counts, value,
                                           value_out, i64(value_bytes), ws, wsb, None)


def _coalesce(row=fake, col=fake, E=9000, M=300, N=500, row_tmp=fake, col_tmp=fake, row_u=fake, col_u=fake, seg=fake,
              counts=fake, value=None, value_out=None, value_bytes=0, ws=fake, wsb=BIG):
    return nat.lib().tsamd_sort_coalesce(row, col, i64(E), i64(M), i64(N), row_tmp, col_tmp, row_u, col_u, seg, counts,
                                         value, value_out, i64(value_bytes), ws, wsb, None)


def _reduce(row=fake, col=fake, E=9000, M=300, N=500, row_tmp=fake, col_tmp=fake, row_u=fake, col_u=fake, seg=fake,
            counts=fake, dtype=0, reduce=0, value=None, value_out=None, value_u=None, ws=fake, wsb=BIG):
    return nat.lib().tsamd_sort_coalesce_reduce(row, col, i64(E), i64(M), i64(N), row_tmp, col_tmp, row_u, col_u, seg,
                                                counts, dtype, reduce, value, value_out, value_u, ws, wsb, None)


ENTRIES = {
    'sort_coo': _sort_coo,
    'sort_coo_auto': lambda **kw: _auto('tsamd_sort_coo_auto', **kw),
    'sort_coo_probed': lambda **kw: _auto('tsamd_sort_coo_probed', **kw),
    'sort_coo_values0': lambda **kw: _values(mode=0, **kw),
    'sort_coo_values1': lambda **kw: _values(mode=1, **kw),
    'sort_coo_values2': lambda **kw: _values(mode=2, **kw),
    'sort_coo_values3': lambda **kw: _values(mode=3, **kw),
    'sort_coalesce': _coalesce,
    'sort_coalesce_reduce': _reduce,
}


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_status_codes_common(name):
    f = ENTRIES[name]
    assert f(E=-1) == 1 and f(M=-1) == 1 and f(N=-1) == 1
    assert f(row=None) == 1 and f(col=None) == 1
    assert f(row=None, E=5) == 1 and f(col=None, E=5) == 1          # also where the one-launch sort would apply
    if 'coalesce' not in name:
        assert f(perm=None) == 1 and f(perm=None, E=5) == 1
    assert f(M=1 << 40, N=1 << 40) == 2 and f(E=5, M=1 << 40, N=1 << 40) == 2
    assert f(row=None, M=1 << 40, N=1 << 40) == 1                   # a null pointer is reported first
    assert f(ws=None, wsb=sz(0)) == 4 and f(wsb=sz(4096)) == 4


def test_status_codes_auto_and_probed():
    for name in ('tsamd_sort_coo_auto', 'tsamd_sort_coo_probed'):
        assert _auto(name, counts=None) == 1
        assert _auto(name, counts=None, E=0) == 1 and _auto(name, counts=None, E=5) == 1
        assert _auto(name, E=9000, M=9, N=9, ws=None, wsb=sz(0)) == 4
        assert _auto(name, E=9000, M=9, N=9, wsb=sz(100)) == 4
    assert _auto('tsamd_sort_coo_probed', E=0) == 0   # (no probe: nothing to write)
    assert _sort_coo(E=0) == 0 and _sort_coo(E=0, row=None, col=None, perm=None, ws=None, wsb=sz(0)) == 0
    assert _sort_coo(E=5, M=9, N=9, ws=None, wsb=sz(0)) == 4   # tsamd_sort_coo wants its workspace at any size


def test_status_codes_values():
    assert _values(mode=-1) == 1 and _values(mode=4) == 1
    assert _values(mode=-1, E=0) == 1 and _values(mode=4, E=0) == 1
    for mode in (1, 2, 3):
        assert _values(mode=mode, counts=None) == 1 and _values(mode=mode, counts=None, E=0) == 1
    assert _values(mode=0, counts=None, ws=None, wsb=sz(0)) == 4   # (mode 0 needs no counts: on to the next check)
    for mode in (0, 1, 2, 3):
        assert _values(mode=mode, value=fake, value_bytes=4) == 1
        assert _values(mode=mode, value_out=fake, value_bytes=4) == 1
        assert _values(mode=mode, value=fake, value_out=fake, value_bytes=2) == 2
        assert _values(mode=mode, value=fake, value_out=fake, value_bytes=2, E=0) == 2
        assert _values(mode=mode, value=fake, value_out=fake, value_bytes=4, M=1 << 40, N=1 << 40) == 2
        assert _values(mode=mode, ws=None, wsb=sz(0)) == 4
        assert _values(mode=mode, E=5, ws=None, wsb=sz(0)) == 4 and _values(mode=mode, E=5, wsb=sz(100)) == 4
        assert _values(mode=mode, E=5, value=fake, value_out=fake, value_bytes=8, ws=None, wsb=sz(0)) == 4
    for mode in (0, 2):
        assert _values(mode=mode, E=0) == 0
        assert _values(mode=mode, E=0, row=None, col=None, perm=None, ws=None, wsb=sz(0)) == 0


def test_status_codes_coalesce():
    for f in (_coalesce, _reduce):
        assert f(counts=None) == 1 and f(seg=None) == 1
        assert f(counts=None, E=0) == 1 and f(seg=None, E=0) == 1
        for tmp in ('row_tmp', 'col_tmp', 'row_u', 'col_u'):
            assert f(**{tmp: None}) == 1 and f(**{tmp: None, 'E': 5}) == 1
        assert f(E=5, ws=None, wsb=sz(0)) == 4 and f(E=5, wsb=sz(4096)) == 4
    assert _coalesce(value=fake, value_bytes=4) == 1 and _coalesce(value_out=fake, value_bytes=4) == 1
    assert _coalesce(value=fake, value_out=fake, value_bytes=2) == 2
    assert _coalesce(value=fake, value_out=fake, value_bytes=2, E=0) == 2
    assert _coalesce(value=fake, value_out=fake, value_bytes=8, ws=None, wsb=sz(0)) == 4
    assert _reduce(reduce=4) == 2 and _reduce(reduce=-1) == 2
    for dtype in (1, 2, 3, 5, 99):   # everything but TSAMD_F32 = 0 / TSAMD_I32 = 4
        assert _reduce(dtype=dtype) == 2
    assert _reduce(dtype=4, ws=None, wsb=sz(0)) == 4
    assert _reduce(reduce=4, counts=None) == 2   # reduce and dtype are looked at first
    for present in ((fake, fake, None), (fake, None, fake), (None, fake, fake), (fake, None, None), (None, fake, None),
                    (None, None, fake)):
        assert _reduce(value=present[0], value_out=present[1], value_u=present[2]) == 1
    assert _reduce(value=fake, value_out=fake, value_u=fake, ws=None, wsb=sz(0)) == 4
