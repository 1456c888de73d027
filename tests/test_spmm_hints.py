"""Pattern hints of the SpMM forward (docs/design/spmm_forward.md, "Pattern hints"): the layout of the hints buffer
and its scope, pinned through tsamd_spmm_hints_layout / tsamd_spmm_hints_bytes with literals -- host arithmetic only,
runs without a GPU.  The parts, each on a 256-byte boundary: the probe's four counters, the order header (64 words),
the 128 chunk totals, one block word per 64 ids, the per-chunk lists (as many words), the slot -> partition map [P].
Whoever moves the partition planner, kHotBlockMinN or relabel_possible revisits these numbers knowingly."""
import ctypes

import torch

from pytorch_sparse_amd import _native as nat

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
E20 = 1 << 20


def test_layout_of_the_smallest_shape():
    # M + E = 1114112 items in partitions of 128 (the floor): P = 8704; 1024 blocks of 64 ids
    lay = nat.spmm_hints_layout(F32, 'sum', 1, 65536, 65536, 64, E20)
    assert lay == dict(flags_off=0, hdr_off=256, totals_off=512, words_off=1024, lists_off=5120, order_off=9216, P=8704,
                       bytes=44032)
    assert nat.spmm_hints_bytes(F32, 'sum', 1, 65536, 65536, 64, E20) == 44032
    assert lay['P'] == nat.spmm_route(F32, 'sum', 1, 65536, 65536, 64, E20)['P']


def test_layout_with_a_partial_last_block():
    # N = 65536 + 41: 1025 block words, padded to 4352 bytes; P = 2105344 / 128 = 16448
    lay = nat.spmm_hints_layout(F32, 'sum', 1, 8192, 65536 + 41, 64, 1 << 21)
    assert lay == dict(flags_off=0, hdr_off=256, totals_off=512, words_off=1024, lists_off=5376, order_off=9728, P=16448,
                       bytes=75520)


def test_mean_and_the_other_types_share_the_layout():
    want = nat.spmm_hints_layout(F32, 'sum', 1, 65536, 65536, 64, E20)
    assert nat.spmm_hints_layout(F32, 'mean', 1, 65536, 65536, 64, E20) == want
    assert nat.spmm_hints_layout(F64, 'sum', 1, 65536, 65536, 32, E20) == want
    assert nat.spmm_hints_layout(BF16, 'sum', 1, 65536, 65536, 128, E20) == want


def test_the_headline_shape_stays_under_a_megabyte():
    # scale 21, at most 20 entries per row: partitions of 256 items, P = 172032; 32768 block words
    n, e = 1 << 21, 20 << 21
    lay = nat.spmm_hints_layout(F32, 'sum', 1, n, n, 128, e)
    assert lay['P'] == 172032 and lay['order_off'] == 1024 + 2 * 131072 and lay['bytes'] == 951296 < (1 << 20)


def test_out_of_scope():
    for args in [(F32, 'sum', 1, 5000, 9001, 64, 1300000),      # the per-id hot route
                 (F32, 'sum', 1, 65536, 65535, 64, E20),        # one id short of kHotBlockMinN
                 (F32, 'max', 1, 65536, 65536, 64, E20), (F32, 'min', 1, 65536, 65536, 64, E20),
                 (F32, 'sum', 2, 65536, 65536, 64, E20),        # two matrices: the full copy
                 (F32, 'sum', 1, 65536, 65536, 64, E20 - 1),    # relabel_possible: E >= 2^20
                 (F32, 'sum', 1, 65536, 131073, 64, E20),       # ... and E >= 8 N
                 (F32, 'sum', 1, 65536, 65536, 96, E20),        # 384-byte rows: no power of two
                 (F32, 'sum', 1, 65536, 65536, 32, E20),        # 128-byte rows
                 (torch.int32, 'sum', 1, 65536, 65536, 64, E20),
                 (F32, 'sum', 1, 0, 65536, 64, E20)]:
        assert nat.spmm_hints_bytes(*args) == 0 and nat.spmm_hints_layout(*args) is None, args


def test_refusals_come_before_any_device_work():
    """out of scope: TSAMD_ERR_UNSUPPORTED (2); no buffer or a state other than 1 / 2: TSAMD_ERR_INVALID (1)"""
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    A = 1 << 30

    def status(reduce, N, hints, state):
        return nat.lib().tsamd_spmm_hinted(0, nat.REDUCES[reduce], vp(A), vp(2 * A), vp(0), vp(3 * A), vp(4 * A), vp(5 * A),
                                           i64(1), i64(65536), i64(N), i64(64), i64(E20), vp(6 * A), ctypes.c_size_t(1 << 40),
                                           vp(hints), ctypes.c_int(state), vp(0))
    assert status('sum', 9001, 7 * A, 1) == 2
    assert status('max', 65536, 7 * A, 2) == 2
    assert status('sum', 65536, 0, 1) == 1
    assert status('sum', 65536, 7 * A, 0) == 1 and status('sum', 65536, 7 * A, 3) == 1
    assert status('sum', 65536, 7 * A + 8, 1) == 1  # off a 256-byte boundary
