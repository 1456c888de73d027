"""The SpSpMM route table (tsamd_spspmm_route, csrc/spspmm.hip: spspmm_route) pinned at every threshold and its
neighbours, for fp32 and fp64 -- host arithmetic only, runs without a GPU.  The expected values below are written out
as literals on purpose: whoever changes TSAMD_SPSPMM_LG_RANGE, kMaxRanges, kOffLdsMax or the key layout of the small
rows has to revisit this table (and tests/test_spspmm_wide_gpu.py, which names its regimes through it) knowingly.
Also: the seeded generator of tests/spspmm_cases.py reaches the routes it claims to (host census)."""
import ctypes

import pytest

from pytorch_sparse_amd import _native as nat

F32, F64 = 0, 1
FIELDS = ('lg_range', 'nr', 'sub', 'off_lds', 'small_pairs', 'passes', 'narrow_hash', 'large_ok')


def route(dtype, N):
    out = (ctypes.c_int64 * 8)()
    st = nat.lib().tsamd_spspmm_route(dtype, ctypes.c_int64(N), out)
    assert st == 0, (dtype, N, st)
    return dict(zip(FIELDS, (int(x) for x in out)))


# (N, lg_range, nr, sub, off_lds, small_pairs, passes, narrow_hash, large_ok)
TABLE = {
    F32: [
        (1,            13, 1,      4, 1, 0, 1, 1, 1),
        (2,            13, 1,      4, 1, 0, 1, 1, 1),
        (97,           13, 1,      4, 1, 0, 1, 1, 1),
        (256,          13, 1,      4, 1, 0, 1, 1, 1),
        (257,          13, 1,      4, 1, 0, 2, 1, 1),
        (1 << 13,      13, 1,      4, 1, 0, 2, 1, 1),
        ((1 << 13) + 1, 13, 2,     4, 1, 0, 2, 1, 1),
        (2 << 13,      13, 2,      4, 1, 0, 2, 1, 1),   # the grid of tests/test_spspmm_narrow_gpu.py: R = 2^13, R + 1, 2R,
        ((2 << 13) + 1, 13, 3,     4, 1, 0, 2, 1, 1),   # 2R + 1, 8R, 15R - 3, 16R, config 4's 500 000, 2^21, 2^22
        (1 << 16,      13, 8,      4, 1, 0, 2, 1, 1),
        ((1 << 16) + 1, 13, 9,     4, 1, 0, 3, 1, 1),
        ((15 << 13) - 3, 13, 15,   4, 1, 0, 3, 1, 1),
        (16 << 13,     13, 16,     4, 1, 0, 3, 1, 1),
        (500000,       13, 62,     4, 1, 0, 3, 1, 1),
        (1 << 21,      13, 256,    4, 1, 0, 3, 1, 1),   # 256 ranges: the last N at which no group can close by span
        (1 << 22,      13, 512,    4, 1, 0, 3, 1, 1),
        ((1 << 23) - 1, 13, 1024,  4, 1, 0, 3, 1, 1),
        (1 << 23,      13, 1024,   4, 1, 0, 3, 1, 1),   # last N with 32-bit (column << 9 | index) keys, offsets in LDS
        ((1 << 23) + 1, 13, 1025,  4, 0, 1, 3, 1, 1),   # pairs radix sort; 4100 segment offsets stay in global memory
        ((1 << 24) - 1, 13, 2048,  4, 0, 1, 3, 1, 1),
        (1 << 24,      13, 2048,   4, 0, 1, 3, 1, 1),   # last N with per-wave segments, 3 passes, 24-bit hash multiply
        ((1 << 24) + 1, 13, 2049,  1, 1, 1, 4, 0, 1),   # shared cursors (2049 of them: offsets back in LDS), 4 passes
        (1 << 25,      13, 4096,   1, 1, 1, 4, 0, 1),
        ((1 << 25) + 1, 13, 4097,  1, 0, 1, 4, 0, 1),
        ((1 << 26) - 1, 13, 8192,  1, 0, 1, 4, 0, 1),
        (1 << 26,      13, 8192,   1, 0, 1, 4, 0, 1),   # last N that supports large rows
        ((1 << 26) + 1, 13, 8193,  1, 0, 1, 4, 0, 0),
        ((1 << 32) - 2, 13, 1 << 19, 1, 0, 1, 4, 0, 0),  # largest N: column ids up to 2^32 - 3, next to the sentinel
    ],
    F64: [
        (1,            12, 1,      4, 1, 0, 1, 1, 1),
        (2,            12, 1,      4, 1, 0, 1, 1, 1),
        (97,           12, 1,      4, 1, 0, 1, 1, 1),
        (1 << 12,      12, 1,      4, 1, 0, 2, 1, 1),
        ((1 << 12) + 1, 12, 2,     4, 1, 0, 2, 1, 1),
        (2 << 12,      12, 2,      4, 1, 0, 2, 1, 1),   # the grid of tests/test_spspmm_narrow_gpu.py, R = 2^12
        ((2 << 12) + 1, 12, 3,     4, 1, 0, 2, 1, 1),
        (8 << 12,      12, 8,      4, 1, 0, 2, 1, 1),
        ((15 << 12) - 3, 12, 15,   4, 1, 0, 2, 1, 1),
        (16 << 12,     12, 16,     4, 1, 0, 2, 1, 1),
        (500000,       12, 123,    4, 1, 0, 3, 1, 1),
        (1 << 21,      12, 512,    4, 1, 0, 3, 1, 1),
        ((1 << 22) - 1, 12, 1024,  4, 1, 0, 3, 1, 1),
        (1 << 22,      12, 1024,   4, 1, 0, 3, 1, 1),
        ((1 << 22) + 1, 12, 1025,  4, 0, 0, 3, 1, 1),
        ((1 << 23) - 1, 12, 2048,  4, 0, 0, 3, 1, 1),
        (1 << 23,      12, 2048,   4, 0, 0, 3, 1, 1),
        ((1 << 23) + 1, 12, 2049,  1, 1, 1, 3, 1, 1),
        (1 << 24,      12, 4096,   1, 1, 1, 3, 1, 1),
        ((1 << 24) + 1, 12, 4097,  1, 0, 1, 4, 0, 1),
        ((1 << 25) - 1, 12, 8192,  1, 0, 1, 4, 0, 1),
        (1 << 25,      12, 8192,   1, 0, 1, 4, 0, 1),
        ((1 << 25) + 1, 12, 8193,  1, 0, 1, 4, 0, 0),
        (1 << 26,      12, 1 << 14, 1, 0, 1, 4, 0, 0),
        ((1 << 26) + 1, 12, (1 << 14) + 1, 1, 0, 1, 4, 0, 0),
        ((1 << 32) - 2, 12, 1 << 20, 1, 0, 1, 4, 0, 0),
    ],
}


@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_route_table(dtype):
    for row in TABLE[dtype]:
        assert route(dtype, row[0]) == dict(zip(FIELDS, row[1:])), 'N = %d' % row[0]


def test_route_thresholds_have_exactly_one_step():
    """Between two neighbouring rows of the table nothing else changes: every flag is monotone in N except off_lds,
    which follows nr * sub (<= 4096) and therefore comes back when the sub-bins are given up."""
    for dtype in (F32, F64):
        for f in ('small_pairs', 'passes'):
            vals = [route(dtype, N)[f] for N in (1 << 20, 1 << 23, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, 1 << 30)]
            assert vals == sorted(vals)
        for f in ('sub', 'narrow_hash', 'large_ok'):
            vals = [route(dtype, N)[f] for N in (1 << 20, 1 << 23, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, 1 << 30)]
            assert vals == sorted(vals, reverse=True)
        for N in (1 << 21, (1 << 22) + 1, (1 << 23) + 1, (1 << 24) + 1, 1 << 25, (1 << 25) + 1):
            r = route(dtype, N)
            assert r['off_lds'] == int(r['nr'] * r['sub'] <= 4096)
            assert r['nr'] == -(-N // (1 << r['lg_range']))


def test_route_refuses_what_the_stages_refuse():
    out = (ctypes.c_int64 * 8)()
    L = nat.lib()
    assert L.tsamd_spspmm_route(F32, ctypes.c_int64((1 << 32) - 1), out) == 2  # column ids must stay below the sentinel
    assert L.tsamd_spspmm_route(F32, ctypes.c_int64(1 << 40), out) == 2
    assert L.tsamd_spspmm_route(F32, ctypes.c_int64(-1), out) == 2
    assert L.tsamd_spspmm_route(2, ctypes.c_int64(100), out) == 2              # fp16
    assert L.tsamd_spspmm_route(F32, ctypes.c_int64(100), None) == 1
    assert L.tsamd_spspmm_route(F64, ctypes.c_int64(0), out) == 0 and list(out)[:3] == [12, 1, 4]


@pytest.mark.parametrize('N', [(1 << 22) + 1, (1 << 23) + 1, 1 << 26])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['fp32', 'fp64'])
def test_generated_case_reaches_every_route(dtype, N):
    """The wide-product generator: deterministic, and its census holds (a (row, range) bin above 1024 products, a
    large row whose groups close by span alone, one that closes a group by the 1024-product cap, every exact row)."""
    import numpy as np
    from tests import spspmm_cases as sc
    lg = route(dtype, N)['lg_range']
    case = sc.make_case(N, lg, seed=0)
    sc.assert_reaches_every_route(case)
    again = sc.make_case(N, lg, seed=0)
    assert np.array_equal(case['colB'], again['colB']) and np.array_equal(case['colA'], again['colA'])
    other = sc.make_case(N, lg, seed=1)
    assert not np.array_equal(case['colB'], other['colB'])
    none = sc.make_case(N, lg, seed=0, large='none')
    assert none['census']['n_large'] == 0 and none['census']['n_medium'] >= 1 and none['census']['n_small'] >= 1
    assert sc.make_case(N, lg, seed=0, large='one')['census']['n_large'] == 1
