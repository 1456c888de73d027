"""The routes and workspace sizes of the segmented kernels (csrc/segtile.h and the units on top of it) pinned for
f32 / f64 / f16 / bf16 -- host arithmetic only, runs without a GPU, nothing is dereferenced (operand pointers are
integer addresses).  The expected values are written out as literals on purpose: the size queries and the launchers
read one layout description (SegRecords), and whoever changes it, a chunk length or a lane map has to revisit these
tables knowingly.

  tsamd_segment_softmax_route, tsamd_sddmm_heads_route, tsamd_spmm_heads_route, tsamd_attention_heads_route,
  tsamd_spspmm_bw_route; tsamd_segment_reduce_balanced_workspace_bytes, tsamd_segment_softmax_workspace_bytes,
  tsamd_spmm_heads_workspace_bytes, tsamd_attention_heads_workspace_bytes, tsamd_spspmm_bw_workspace_bytes.

(H, D) grid: (1, 1), (3, 5), (4, 16), (16, 64), (17, 8), (1, 64 VEC), (1, 64 VEC + 1) -- the first fblocks = 2 of the
fused attention, VEC = 16 / itemsize -- and (2, 4) with one operand off the 16-byte boundary.  E grid of the sizes:
0, 1, 511, 512, 513, 2048, 2049, 10^6.  The segment reductions and the softmax take H as their D (columns)."""
import ctypes

import pytest

from pytorch_sparse_amd import _native as nat

F32, F64, F16, BF16 = 0, 1, 2, 3
DTYPES = (F32, F64, F16, BF16)
NAMES = {F32: 'F32', F64: 'F64', F16: 'F16', BF16: 'BF16'}
ITEMSIZE = {F32: 4, F64: 8, F16: 2, BF16: 2}
ENTRIES = (0, 1, 511, 512, 513, 2048, 2049, 10 ** 6)
EXPORTS = ('segment_reduce', 'segment_softmax', 'spmm_heads', 'attention_heads')
ALIGNED, OFF = 1 << 20, (1 << 20) + 4  # operand addresses: on and off the 16-byte boundary

i64, vp, i64p = ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)


def declare(L):
    L.tsamd_segment_softmax_route.argtypes = [i64p]
    L.tsamd_spspmm_bw_route.argtypes = [ctypes.c_int, i64p]
    L.tsamd_sddmm_heads_route.argtypes = [ctypes.c_int, i64, i64, vp, vp, i64p]
    L.tsamd_spmm_heads_route.argtypes = [ctypes.c_int, i64, i64, vp, vp, i64p]
    L.tsamd_attention_heads_route.argtypes = [ctypes.c_int, i64, i64, vp, vp, vp, vp, i64p]
    for name, args in (('tsamd_segment_reduce_balanced_workspace_bytes', [ctypes.c_int, i64, i64]),
                       ('tsamd_segment_softmax_workspace_bytes', [ctypes.c_int, i64, i64]),
                       ('tsamd_spmm_heads_workspace_bytes', [ctypes.c_int, i64, i64, i64, i64]),
                       ('tsamd_attention_heads_workspace_bytes', [ctypes.c_int, i64, i64, i64]),
                       ('tsamd_spspmm_bw_workspace_bytes', [ctypes.c_int, i64])):
        getattr(L, name).argtypes = args
        getattr(L, name).restype = ctypes.c_size_t
    return L


def grid(dtype):
    vec = 16 // ITEMSIZE[dtype]
    return [(1, 1, 0), (3, 5, 0), (4, 16, 0), (16, 64, 0), (17, 8, 0), (1, 64 * vec, 0), (1, 64 * vec + 1, 0),
            (2, 4, 1)]


def _route(fn, *args):
    out = (ctypes.c_int64 * 8)()
    st = fn(*args, out)
    return (st,) + tuple(int(x) for x in out)


def softmax_route(L):
    return _route(L.tsamd_segment_softmax_route)


def spspmm_bw_route(L, dtype):
    return _route(L.tsamd_spspmm_bw_route, dtype)


def heads_routes(L, dtype, H, D, off):
    """sddmm (k off the boundary), spmm_heads (out off), attention (v off) when `off`."""
    last = OFF if off else ALIGNED
    return (_route(L.tsamd_sddmm_heads_route, dtype, H, D, ALIGNED, last),
            _route(L.tsamd_spmm_heads_route, dtype, H, D, ALIGNED, last),
            _route(L.tsamd_attention_heads_route, dtype, H, D, ALIGNED, ALIGNED, last, ALIGNED))


def workspaces(L, dtype, H, D):
    return {
        'segment_reduce': tuple(int(L.tsamd_segment_reduce_balanced_workspace_bytes(dtype, E, H)) for E in ENTRIES),
        'segment_softmax': tuple(int(L.tsamd_segment_softmax_workspace_bytes(dtype, E, H)) for E in ENTRIES),
        'spmm_heads': tuple(int(L.tsamd_spmm_heads_workspace_bytes(dtype, 1000, H, D, E)) for E in ENTRIES),
        'attention_heads': tuple(int(L.tsamd_attention_heads_workspace_bytes(dtype, H, D, E)) for E in ENTRIES),
    }


def spspmm_bw_workspace(L, dtype):
    return tuple(int(L.tsamd_spspmm_bw_workspace_bytes(dtype, P)) for P in ENTRIES)


# ---- the tables: (status, out[0..7]) per route --------------------------------------------------------------------
SOFTMAX_ROUTE = (0, 512, 2048, 2048, 64, 0, 0, 0, 0)
SPSPMM_BW_ROUTE = {
    F32: (0, 2048, 2048, 512, 2, 0, 0, 0, 0),
    F64: (0, 2048, 2048, 512, 2, 0, 0, 0, 0),
    F16: (2, 0, 0, 0, 0, 0, 0, 0, 0),
    BF16: (2, 0, 0, 0, 0, 0, 0, 0, 0),
}
# (H, D, off): sddmm route, spmm_heads route, attention route
ROUTES = {
    F32: [
        (1, 1, 0, (0, 1, 1, 1, 64, 1, 64, 256, 16),
         (0, 1, 1, 1, 64, 8, 2048, 2048, 1),
         (0, 1, 1, 1, 1, 1, 8, 2048, 1)),
        (3, 5, 0, (0, 1, 1, 8, 2, 4, 64, 256, 16),
         (0, 1, 1, 4, 16, 32, 2048, 2048, 4),
         (0, 1, 1, 2, 4, 1, 64, 2048, 1)),
        (4, 16, 0, (0, 0, 4, 4, 4, 4, 64, 256, 16),
         (0, 0, 4, 16, 4, 128, 2048, 2048, 1),
         (0, 0, 4, 4, 4, 1, 128, 2048, 1)),
        (16, 64, 0, (0, 0, 4, 16, 1, 4, 64, 256, 16),
         (0, 0, 4, 64, 1, 512, 2048, 2048, 4),
         (0, 0, 4, 16, 4, 4, 512, 2048, 1)),
        (17, 8, 0, (0, 0, 4, 2, 2, 16, 64, 256, 16),
         (0, 0, 4, 64, 1, 512, 2048, 2048, 1),
         (0, 0, 4, 2, 32, 1, 512, 2048, 1)),
        (1, 256, 0, (0, 0, 4, 64, 1, 1, 64, 256, 16),
         (0, 0, 4, 64, 1, 512, 2048, 2048, 1),
         (0, 0, 4, 64, 1, 1, 512, 2048, 1)),
        (1, 257, 0, (0, 1, 1, 64, 1, 1, 64, 256, 16),
         (0, 1, 1, 64, 1, 512, 2048, 2048, 5),
         (0, 1, 1, 64, 1, 2, 512, 2048, 2)),
        (2, 4, 1, (0, 1, 1, 4, 8, 2, 64, 256, 16),
         (0, 1, 1, 2, 32, 16, 2048, 2048, 4),
         (0, 1, 1, 1, 2, 1, 16, 2048, 1)),
    ],
    F64: [
        (1, 1, 0, (0, 1, 1, 1, 64, 1, 64, 256, 16),
         (0, 1, 1, 1, 64, 8, 2048, 2048, 1),
         (0, 1, 1, 1, 1, 1, 8, 2048, 1)),
        (3, 5, 0, (0, 1, 1, 8, 2, 4, 64, 256, 16),
         (0, 1, 1, 8, 8, 64, 2048, 2048, 2),
         (0, 1, 1, 4, 4, 1, 128, 2048, 1)),
        (4, 16, 0, (0, 0, 2, 8, 2, 4, 64, 256, 16),
         (0, 0, 2, 32, 2, 256, 2048, 2048, 1),
         (0, 0, 2, 8, 4, 1, 256, 2048, 1)),
        (16, 64, 0, (0, 0, 2, 32, 1, 2, 64, 256, 16),
         (0, 0, 2, 64, 1, 512, 2048, 2048, 8),
         (0, 0, 2, 32, 2, 8, 512, 2048, 1)),
        (17, 8, 0, (0, 0, 2, 4, 1, 16, 64, 256, 16),
         (0, 0, 2, 64, 1, 512, 2048, 2048, 2),
         (0, 0, 2, 4, 16, 2, 512, 2048, 1)),
        (1, 128, 0, (0, 0, 2, 64, 1, 1, 64, 256, 16),
         (0, 0, 2, 64, 1, 512, 2048, 2048, 1),
         (0, 0, 2, 64, 1, 1, 512, 2048, 1)),
        (1, 129, 0, (0, 1, 1, 64, 1, 1, 64, 256, 16),
         (0, 1, 1, 64, 1, 512, 2048, 2048, 3),
         (0, 1, 1, 64, 1, 2, 512, 2048, 2)),
        (2, 4, 1, (0, 1, 1, 4, 8, 2, 64, 256, 16),
         (0, 1, 1, 4, 16, 32, 2048, 2048, 2),
         (0, 1, 1, 2, 2, 1, 32, 2048, 1)),
    ],
    F16: [
        (1, 1, 0, (0, 1, 1, 1, 64, 1, 64, 256, 16),
         (0, 1, 1, 1, 64, 8, 2048, 2048, 1),
         (0, 1, 1, 1, 1, 1, 8, 2048, 1)),
        (3, 5, 0, (0, 1, 1, 8, 2, 4, 64, 256, 16),
         (0, 1, 1, 2, 32, 16, 2048, 2048, 8),
         (0, 1, 1, 1, 4, 1, 32, 2048, 1)),
        (4, 16, 0, (0, 0, 8, 2, 8, 4, 64, 256, 16),
         (0, 0, 8, 8, 8, 64, 2048, 2048, 1),
         (0, 0, 8, 2, 4, 1, 64, 2048, 1)),
        (16, 64, 0, (0, 0, 8, 8, 1, 8, 64, 256, 16),
         (0, 0, 8, 64, 1, 512, 2048, 2048, 2),
         (0, 0, 8, 8, 8, 2, 512, 2048, 1)),
        (17, 8, 0, (0, 0, 8, 1, 4, 16, 64, 256, 16),
         (0, 0, 8, 32, 2, 256, 2048, 2048, 1),
         (0, 0, 8, 1, 32, 1, 256, 2048, 1)),
        (1, 512, 0, (0, 0, 8, 64, 1, 1, 64, 256, 16),
         (0, 0, 8, 64, 1, 512, 2048, 2048, 1),
         (0, 0, 8, 64, 1, 1, 512, 2048, 1)),
        (1, 513, 0, (0, 1, 1, 64, 1, 1, 64, 256, 16),
         (0, 1, 1, 64, 1, 512, 2048, 2048, 9),
         (0, 1, 1, 64, 1, 2, 512, 2048, 2)),
        (2, 4, 1, (0, 1, 1, 4, 8, 2, 64, 256, 16),
         (0, 1, 1, 1, 64, 8, 2048, 2048, 8),
         (0, 1, 1, 1, 2, 1, 16, 2048, 1)),
    ],
    BF16: [
        (1, 1, 0, (0, 1, 1, 1, 64, 1, 64, 256, 16),
         (0, 1, 1, 1, 64, 8, 2048, 2048, 1),
         (0, 1, 1, 1, 1, 1, 8, 2048, 1)),
        (3, 5, 0, (0, 1, 1, 8, 2, 4, 64, 256, 16),
         (0, 1, 1, 2, 32, 16, 2048, 2048, 8),
         (0, 1, 1, 1, 4, 1, 32, 2048, 1)),
        (4, 16, 0, (0, 0, 8, 2, 8, 4, 64, 256, 16),
         (0, 0, 8, 8, 8, 64, 2048, 2048, 1),
         (0, 0, 8, 2, 4, 1, 64, 2048, 1)),
        (16, 64, 0, (0, 0, 8, 8, 1, 8, 64, 256, 16),
         (0, 0, 8, 64, 1, 512, 2048, 2048, 2),
         (0, 0, 8, 8, 8, 2, 512, 2048, 1)),
        (17, 8, 0, (0, 0, 8, 1, 4, 16, 64, 256, 16),
         (0, 0, 8, 32, 2, 256, 2048, 2048, 1),
         (0, 0, 8, 1, 32, 1, 256, 2048, 1)),
        (1, 512, 0, (0, 0, 8, 64, 1, 1, 64, 256, 16),
         (0, 0, 8, 64, 1, 512, 2048, 2048, 1),
         (0, 0, 8, 64, 1, 1, 512, 2048, 1)),
        (1, 513, 0, (0, 1, 1, 64, 1, 1, 64, 256, 16),
         (0, 1, 1, 64, 1, 512, 2048, 2048, 9),
         (0, 1, 1, 64, 1, 2, 512, 2048, 2)),
        (2, 4, 1, (0, 1, 1, 4, 8, 2, 64, 256, 16),
         (0, 1, 1, 1, 64, 8, 2048, 2048, 8),
         (0, 1, 1, 1, 2, 1, 16, 2048, 1)),
    ],
}
# (H, D): bytes at E = (0, 1, 511, 512, 513, 2048, 2049, 1000000)
WORKSPACE = {
    F32: [
        (1, 1, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (1024, 1024, 1536, 1536, 2560, 6144, 7168, 3000832),
            'attention_heads': (1536, 1536, 2560, 2560, 4096, 10240, 11776, 5001216),
        }),
        (3, 5, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 78848),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 173056),
            'spmm_heads': (1024, 1024, 2560, 2560, 2560, 8704, 9728, 4250624),
            'attention_heads': (1536, 1536, 2048, 2048, 2560, 6144, 7168, 2875904),
        }),
        (4, 16, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 94720),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 219904),
            'spmm_heads': (1024, 1024, 2560, 2560, 3072, 8704, 9216, 4125696),
            'attention_heads': (1536, 1536, 3072, 3072, 3584, 9728, 10752, 4625920),
        }),
        (16, 64, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1536, 282112),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 2048, 2816, 782080),
            'spmm_heads': (8704, 8704, 8704, 8704, 16896, 33280, 41472, 16038912),
            'attention_heads': (9216, 9216, 9216, 9216, 17408, 34304, 43008, 16539136),
        }),
        (17, 8, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1536, 1536, 297984),
            'segment_softmax': (1280, 1280, 1280, 1280, 2048, 2816, 2816, 829696),
            'spmm_heads': (2048, 2048, 2048, 2048, 3072, 5120, 6144, 2158080),
            'attention_heads': (2560, 2560, 2560, 2560, 4096, 6656, 7680, 2690048),
        }),
        (1, 256, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (2560, 2560, 2560, 2560, 4608, 8704, 10752, 4033536),
            'attention_heads': (3072, 3072, 3072, 3072, 5120, 9216, 11264, 4065280),
        }),
        (1, 257, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (3072, 3072, 3072, 3072, 5120, 9216, 11264, 4049408),
            'attention_heads': (3584, 3584, 3584, 3584, 5632, 9728, 11776, 4081152),
        }),
    ],
    F64: [
        (1, 1, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 63488),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 126208),
            'spmm_heads': (1024, 1024, 2048, 2048, 3072, 8192, 9216, 4000768),
            'attention_heads': (1536, 1536, 4096, 4096, 5632, 16384, 17920, 8001024),
        }),
        (3, 5, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 125952),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 313600),
            'spmm_heads': (1024, 1024, 2560, 2560, 3072, 8192, 9216, 4000768),
            'attention_heads': (1536, 1536, 2048, 2048, 2560, 6144, 6656, 2750976),
        }),
        (4, 16, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 157184),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 2048, 407296),
            'spmm_heads': (1536, 1536, 2560, 2560, 3584, 8704, 9728, 4063744),
            'attention_heads': (2048, 2048, 3072, 3072, 4096, 9728, 11264, 4563968),
        }),
        (16, 64, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1536, 2048, 531968),
            'segment_softmax': (1280, 1280, 1280, 1280, 2048, 3584, 4352, 1532416),
            'spmm_heads': (16896, 16896, 16896, 16896, 33280, 66048, 82432, 32046080),
            'attention_heads': (17408, 17408, 17408, 17408, 34304, 68096, 84992, 33046528),
        }),
        (17, 8, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1536, 2048, 2048, 563712),
            'segment_softmax': (2048, 2048, 2048, 2048, 2816, 4352, 5120, 1626880),
            'spmm_heads': (3072, 3072, 3072, 3072, 5120, 9216, 11776, 4283904),
            'attention_heads': (4096, 4096, 4096, 4096, 6656, 11776, 14848, 5347328),
        }),
        (1, 128, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 63488),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 126208),
            'spmm_heads': (2560, 2560, 2560, 2560, 4608, 8704, 10752, 4033536),
            'attention_heads': (3072, 3072, 3072, 3072, 5120, 9216, 11264, 4096512),
        }),
        (1, 129, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 63488),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 126208),
            'spmm_heads': (3072, 3072, 3072, 3072, 5120, 9216, 11264, 4065280),
            'attention_heads': (3584, 3584, 3584, 3584, 5632, 9728, 11776, 4128256),
        }),
    ],
    F16: [
        (1, 1, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (1024, 1024, 1536, 1536, 2560, 6144, 7168, 3000832),
            'attention_heads': (1536, 1536, 2560, 2560, 4096, 10240, 11776, 5001216),
        }),
        (3, 5, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 78848),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 173056),
            'spmm_heads': (1024, 1024, 4608, 4608, 5120, 17408, 18432, 8500736),
            'attention_heads': (1536, 1536, 3584, 3584, 3584, 11776, 13312, 5750784),
        }),
        (4, 16, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 94720),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 219904),
            'spmm_heads': (1024, 1024, 4608, 4608, 5120, 16896, 17920, 8250368),
            'attention_heads': (1536, 1536, 5120, 5120, 6144, 18944, 20480, 9250816),
        }),
        (16, 64, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1536, 282112),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 2048, 2816, 782080),
            'spmm_heads': (8704, 8704, 8704, 8704, 16896, 33280, 41472, 16038912),
            'attention_heads': (9216, 9216, 9216, 9216, 17408, 34304, 43008, 16539136),
        }),
        (17, 8, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1536, 1536, 297984),
            'segment_softmax': (1280, 1280, 1280, 1280, 2048, 2816, 2816, 829696),
            'spmm_heads': (2048, 2048, 3072, 3072, 4096, 9216, 10752, 4314112),
            'attention_heads': (2560, 2560, 4096, 4096, 5120, 11776, 13312, 5377024),
        }),
        (1, 512, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (4608, 4608, 4608, 4608, 8704, 16896, 20992, 8035328),
            'attention_heads': (5120, 5120, 5120, 5120, 9216, 17408, 21504, 8067072),
        }),
        (1, 513, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (5120, 5120, 5120, 5120, 9216, 17408, 21504, 8051200),
            'attention_heads': (5632, 5632, 5632, 5632, 9728, 17920, 22016, 8082944),
        }),
    ],
    BF16: [
        (1, 1, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (1024, 1024, 1536, 1536, 2560, 6144, 7168, 3000832),
            'attention_heads': (1536, 1536, 2560, 2560, 4096, 10240, 11776, 5001216),
        }),
        (3, 5, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 78848),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 173056),
            'spmm_heads': (1024, 1024, 4608, 4608, 5120, 17408, 18432, 8500736),
            'attention_heads': (1536, 1536, 3584, 3584, 3584, 11776, 13312, 5750784),
        }),
        (4, 16, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 94720),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 219904),
            'spmm_heads': (1024, 1024, 4608, 4608, 5120, 16896, 17920, 8250368),
            'attention_heads': (1536, 1536, 5120, 5120, 6144, 18944, 20480, 9250816),
        }),
        (16, 64, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1536, 282112),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 2048, 2816, 782080),
            'spmm_heads': (8704, 8704, 8704, 8704, 16896, 33280, 41472, 16038912),
            'attention_heads': (9216, 9216, 9216, 9216, 17408, 34304, 43008, 16539136),
        }),
        (17, 8, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1536, 1536, 297984),
            'segment_softmax': (1280, 1280, 1280, 1280, 2048, 2816, 2816, 829696),
            'spmm_heads': (2048, 2048, 3072, 3072, 4096, 9216, 10752, 4314112),
            'attention_heads': (2560, 2560, 4096, 4096, 5120, 11776, 13312, 5377024),
        }),
        (1, 512, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (4608, 4608, 4608, 4608, 8704, 16896, 20992, 8035328),
            'attention_heads': (5120, 5120, 5120, 5120, 9216, 17408, 21504, 8067072),
        }),
        (1, 513, {
            'segment_reduce': (1024, 1024, 1024, 1024, 1024, 1024, 1024, 47616),
            'segment_softmax': (1280, 1280, 1280, 1280, 1280, 1280, 1280, 79360),
            'spmm_heads': (5120, 5120, 5120, 5120, 9216, 17408, 21504, 8051200),
            'attention_heads': (5632, 5632, 5632, 5632, 9728, 17920, 22016, 8082944),
        }),
    ],
}
SPSPMM_BW_WORKSPACE = {
    F32: (1024, 1024, 1024, 1024, 1024, 1024, 1024, 12288),
    F64: (1024, 1024, 1024, 1024, 1024, 1024, 1024, 16384),
    F16: (1024, 1024, 1024, 1024, 1024, 1024, 1024, 12288),
    BF16: (1024, 1024, 1024, 1024, 1024, 1024, 1024, 12288),
}


@pytest.fixture(scope='module')
def L():
    return declare(nat.lib())


def test_softmax_and_spspmm_bw_routes(L):
    assert softmax_route(L) == SOFTMAX_ROUTE
    for dtype in DTYPES:
        assert spspmm_bw_route(L, dtype) == SPSPMM_BW_ROUTE[dtype], NAMES[dtype]


@pytest.mark.parametrize('dtype', DTYPES, ids=[NAMES[d] for d in DTYPES])
def test_heads_routes(L, dtype):
    assert [row[:3] for row in ROUTES[dtype]] == grid(dtype)
    for H, D, off, sddmm, spmm, attention in ROUTES[dtype]:
        assert heads_routes(L, dtype, H, D, off) == (sddmm, spmm, attention), (H, D, off)


@pytest.mark.parametrize('dtype', DTYPES, ids=[NAMES[d] for d in DTYPES])
def test_workspace_bytes(L, dtype):
    assert [row[:2] for row in WORKSPACE[dtype]] == [g[:2] for g in grid(dtype) if not g[2]]
    for H, D, want in WORKSPACE[dtype]:
        assert workspaces(L, dtype, H, D) == want, (H, D)
    assert spspmm_bw_workspace(L, dtype) == SPSPMM_BW_WORKSPACE[dtype]


def test_first_two_feature_blocks_are_in_the_grid():
    """(1, 64 VEC) is the last D of one feature block, (1, 64 VEC + 1) the first of two (out_route[7])."""
    for dtype in DTYPES:
        by_hd = {(H, D): att for H, D, off, _, _, att in ROUTES[dtype]}
        vec = 16 // ITEMSIZE[dtype]
        assert by_hd[(1, 64 * vec)][8] == 1 and by_hd[(1, 64 * vec + 1)][8] == 2
