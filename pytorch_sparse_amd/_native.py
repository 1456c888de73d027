"""ctypes binding of the C-ABI in ``include/tsamd.h`` (``lib/libtsamd.so``).

This is the thin layer that hands torch device pointers, sizes and the current
HIP stream to the hand-written kernels.  There is no CPU implementation behind
it: a missing library, a CPU tensor or a non-zero status raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TSAMD_LIB') or os.path.join(_HERE, 'lib', 'libtsamd.so')

# Every symbol include/tsamd.h declares (tests check that all of them resolve).
SYMBOLS = [
    'tsamd_hip_version', 'tsamd_build_flags', 'tsamd_last_hip_error', 'tsamd_status_string',
    'tsamd_spmm_workspace_bytes', 'tsamd_spmm_hot_rows_layout', 'tsamd_spmm_hot_blocks_layout', 'tsamd_spmm_hot_block_min', 'tsamd_spmm_route', 'tsamd_spmm', 'tsamd_spmm_reference_order', 'tsamd_spmm_column_order', 'tsamd_spmm_order_layout', 'tsamd_spmm_permuted', 'tsamd_spmm_profiled',
    'tsamd_spmm_partial_workspace_bytes', 'tsamd_spmm_partial',
    'tsamd_spmm_operand_cache_bytes', 'tsamd_spmm_cached_workspace_bytes', 'tsamd_spmm_cached',
    'tsamd_spmm_hints_bytes', 'tsamd_spmm_hints_layout', 'tsamd_spmm_hinted',
    'tsamd_spmm_minmax_arg32', 'tsamd_spmm_minmax_bw_csc_arg32',
    'tsamd_spmm_minmax_records_in_forward', 'tsamd_spmm_minmax_records_bytes', 'tsamd_spmm_minmax_records_workspace_bytes', 'tsamd_spmm_minmax_records',
    'tsamd_spmm_minmax_winrec', 'tsamd_spmm_minmax_bw_csc_records_workspace_bytes', 'tsamd_spmm_minmax_bw_csc_records',
    'tsamd_gather_rows', 'tsamd_relabel_ids', 'tsamd_spmm_relabelled_workspace_bytes', 'tsamd_spmm_relabelled',
    'tsamd_spmm_coo_small_supported', 'tsamd_spmm_coo_small',
    'tsamd_spmm_value_bw',
    'tsamd_spmm_minmax_bw_workspace_bytes', 'tsamd_spmm_minmax_bw',
    'tsamd_spmm_minmax_bw_csc_workspace_bytes', 'tsamd_spmm_minmax_bw_csc', 'tsamd_spmm_minmax_bw_route',
    'tsamd_ind2ptr', 'tsamd_ptr2ind',
    'tsamd_coo_order', 'tsamd_coo_check', 'tsamd_sort_rank_mode', 'tsamd_sort_route', 'tsamd_sort_header', 'tsamd_sort_coalesce_workspace_bytes', 'tsamd_sort_coalesce', 'tsamd_sort_coalesce_reduce', 'tsamd_sort_coo_workspace_bytes', 'tsamd_sort_coo', 'tsamd_sort_coo_auto', 'tsamd_sort_coo_probed', 'tsamd_sort_coo_values',
    'tsamd_coalesce_workspace_bytes', 'tsamd_coalesce_index', 'tsamd_segment_reduce',
    'tsamd_segment_reduce_balanced_workspace_bytes', 'tsamd_segment_reduce_balanced',
    'tsamd_segment_softmax_route', 'tsamd_segment_softmax_workspace_bytes', 'tsamd_segment_softmax', 'tsamd_segment_softmax_bw',
    'tsamd_sddmm_heads_route', 'tsamd_sddmm_heads', 'tsamd_spmm_heads_route', 'tsamd_spmm_heads_workspace_bytes', 'tsamd_spmm_heads',
    'tsamd_attention_heads_route', 'tsamd_attention_heads_workspace_bytes', 'tsamd_attention_heads', 'tsamd_attention_heads_bw',
    'tsamd_gat_attention_heads', 'tsamd_gat_attention_heads_bw',
    'tsamd_attention_heads_dropout', 'tsamd_attention_heads_dropout_bw', 'tsamd_gat_attention_heads_dropout',
    'tsamd_gat_attention_heads_dropout_bw', 'tsamd_attention_dropout_mask',
    'tsamd_exclusive_scan_workspace_bytes', 'tsamd_exclusive_scan_i64',
    'tsamd_spspmm_route', 'tsamd_spspmm_plan', 'tsamd_spspmm_workspace_bytes', 'tsamd_spspmm_symbolic', 'tsamd_spspmm_numeric',
    'tsamd_spspmm_bw_route', 'tsamd_spspmm_bw_plan_workspace_bytes', 'tsamd_spspmm_bw_workspace_bytes', 'tsamd_spspmm_bw_plan', 'tsamd_spspmm_value_bw',
    'tsamd_index_route', 'tsamd_select_workspace_bytes', 'tsamd_select_plan', 'tsamd_select_fill',
    'tsamd_filter_workspace_bytes', 'tsamd_filter_plan', 'tsamd_filter_apply',
    'tsamd_filter_tiles_workspace_bytes', 'tsamd_filter_count', 'tsamd_filter_write',
    'tsamd_scatter_rows',
    'tsamd_num_diag', 'tsamd_non_diag_mask', 'tsamd_insert_diag', 'tsamd_set_diag_apply',
    'tsamd_random_walk', 'tsamd_sample_workspace_bytes', 'tsamd_sample_plan', 'tsamd_sample_draw',
    'tsamd_relabel_workspace_bytes', 'tsamd_relabel_plan', 'tsamd_relabel_apply', 'tsamd_relabel_seed',
    'tsamd_relabel_extend', 'tsamd_temporal_mark', 'tsamd_temporal_redraw_workspace_bytes', 'tsamd_temporal_redraw',
    'tsamd_temporal_relabel_workspace_bytes', 'tsamd_temporal_relabel', 'tsamd_temporal_emit', 'tsamd_subset_assoc',
    'tsamd_ego_seeds', 'tsamd_ego_plan_workspace_bytes', 'tsamd_ego_plan', 'tsamd_ego_draw', 'tsamd_ego_roots',
    'tsamd_ego_induced_workspace_bytes', 'tsamd_ego_induced_count', 'tsamd_ego_induced_write',
    'tsamd_hgt_seen', 'tsamd_hgt_budget_add', 'tsamd_hgt_select_workspace_bytes', 'tsamd_hgt_select', 'tsamd_hgt_keys',
    'tsamd_hgt_commit', 'tsamd_hgt_check_ids',
    'tsamd_partition_edges', 'tsamd_partition_vertex_weights', 'tsamd_partition_match_workspace_bytes',
    'tsamd_partition_match', 'tsamd_partition_bfs_init', 'tsamd_partition_bfs_seed', 'tsamd_partition_bfs_step',
    'tsamd_partition_assign_workspace_bytes', 'tsamd_partition_assign', 'tsamd_partition_part_weights',
    'tsamd_partition_conn_workspace_bytes', 'tsamd_partition_conn', 'tsamd_partition_recount',
    'tsamd_partition_commit_workspace_bytes', 'tsamd_partition_commit', 'tsamd_partition_apply', 'tsamd_partition_cut',
    'tsamd_partition_keep_better', 'tsamd_partition_balance',
    'tsamd_rcm_limits', 'tsamd_rcm_degree', 'tsamd_rcm_relabel', 'tsamd_rcm_begin', 'tsamd_rcm_small',
    'tsamd_rcm_level_workspace_bytes', 'tsamd_rcm_level_plan', 'tsamd_rcm_level_run', 'tsamd_rcm_finish',
]

DTYPES = {
    torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3,
    torch.int32: 4, torch.int64: 5, torch.uint8: 6, torch.int8: 7, torch.int16: 8,
}
REDUCES = {'sum': 0, 'add': 0, 'mean': 1, 'min': 2, 'max': 3}

_lib = None


class TsamdError(RuntimeError):
    pass


def lib():
    """Load libtsamd.so once; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'pytorch_sparse_amd: %s is missing. Build it with '
                '`python pytorch_sparse_amd/build.py` (needs hipcc, targets gfx950). '
                'There is no CPU fallback.' % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.tsamd_hip_version.restype = ctypes.c_int64
        L.tsamd_status_string.restype = ctypes.c_char_p
        L.tsamd_spmm_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spspmm_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spspmm_bw_plan_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spspmm_bw_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_exclusive_scan_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_partial_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_hints_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_minmax_bw_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_minmax_bw_csc_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_minmax_records_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_minmax_records_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_minmax_bw_csc_records_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_segment_softmax_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_sort_coo_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_sort_coalesce_workspace_bytes.restype = ctypes.c_size_t
        i64, vp, i64p = ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)
        L.tsamd_sddmm_heads_route.argtypes = [ctypes.c_int, i64, i64, vp, vp, i64p]
        L.tsamd_sddmm_heads.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_double, vp, i64, i64, i64, i64, i64, vp]
        L.tsamd_spmm_heads_route.argtypes = [ctypes.c_int, i64, i64, vp, vp, i64p]
        L.tsamd_spmm_heads_workspace_bytes.argtypes = [ctypes.c_int, i64, i64, i64, i64]
        L.tsamd_spmm_heads_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_spmm_heads.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, vp, ctypes.c_size_t, vp]
        L.tsamd_attention_heads_route.argtypes = [ctypes.c_int, i64, i64, vp, vp, vp, vp, i64p]
        L.tsamd_attention_heads_workspace_bytes.argtypes = [ctypes.c_int, i64, i64, i64]
        L.tsamd_attention_heads_workspace_bytes.restype = ctypes.c_size_t
        # the fused calls: dot-product and additive (GAT) scores share their signatures
        fused_fw = [ctypes.c_int, vp, vp, vp, i64, vp, vp, vp, ctypes.c_double, vp, vp, i64, i64, i64, i64, i64, vp, ctypes.c_size_t, vp]
        fused_bw = [ctypes.c_int, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, ctypes.c_double, vp, vp, i64, i64, i64, i64, i64, vp]
        L.tsamd_attention_heads.argtypes = L.tsamd_gat_attention_heads.argtypes = fused_fw
        L.tsamd_attention_heads_bw.argtypes = L.tsamd_gat_attention_heads_bw.argtypes = fused_bw
        # with dropout on the probabilities: (double rate, uint64 seed) after the scalar
        drop = [ctypes.c_double, ctypes.c_uint64]
        L.tsamd_attention_heads_dropout.argtypes = L.tsamd_gat_attention_heads_dropout.argtypes = \
            fused_fw[:9] + drop + fused_fw[9:]
        L.tsamd_attention_heads_dropout_bw.argtypes = L.tsamd_gat_attention_heads_dropout_bw.argtypes = \
            fused_bw[:13] + drop + fused_bw[13:]
        L.tsamd_attention_dropout_mask.argtypes = [ctypes.c_uint64, ctypes.c_double, i64, i64, i64, vp]
        L.tsamd_select_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_filter_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_filter_tiles_workspace_bytes.restype = ctypes.c_size_t
        L.tsamd_num_diag.restype = ctypes.c_int64
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        L = lib()
        msg = L.tsamd_status_string(int(status)).decode()
        if status == 3:
            msg += ' (hipError_t %d)' % L.tsamd_last_hip_error()
        raise TsamdError('%s failed: %s' % (what, msg))


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _i64(x):
    return ctypes.c_int64(int(x))


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise TsamdError(
                'pytorch_sparse_amd runs on MI355X (HIP) tensors only; got a %s tensor. '
                'There is no CPU implementation in this package.' % t.device.type)


def stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dtype):
    try:
        return DTYPES[dtype]
    except KeyError:
        raise TsamdError('unsupported dtype %s (supported: %s)' % (dtype, sorted(map(str, DTYPES))))


def workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def spmm(rowptr, col, value, mat, reduce, out=None, profile=None):
    """C-ABI ``tsamd_spmm``: returns (out, arg_out or None).  mat: [..., N, K] contiguous.
    ``profile``: optional list; receives [partition_ms, merge_ms, fixup_ms] (synchronises)."""
    require_gpu(rowptr, col, value, mat)
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    if value is not None and value.dtype != mat.dtype:
        raise TsamdError('expected scalar type %s but found %s' % (mat.dtype, value.dtype))
    if mat.dim() < 2:
        raise TsamdError('Input mismatch: mat.dim() >= 2 required')
    mat = mat.contiguous()
    M, E = rowptr.numel() - 1, col.numel()
    N, K = mat.size(-2), mat.size(-1)
    B = mat.numel() // max(N * K, 1) if N * K > 0 else 1
    sizes = list(mat.shape)
    sizes[-2] = M
    if out is None:
        out = torch.empty(sizes, dtype=mat.dtype, device=mat.device)
    arg = None
    if red >= 2:
        arg = torch.empty(sizes, dtype=torch.int64, device=mat.device)
    L = lib()
    nb = L.tsamd_spmm_workspace_bytes(dt, red, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E))
    ws = workspace(nb, mat.device)
    with torch.cuda.device(mat.device):
        args = (dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(arg),
                _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), _ptr(ws), ctypes.c_size_t(ws.numel()),
                stream_ptr(mat.device))
        if profile is None:
            st = L.tsamd_spmm(*args)
        else:
            ms = (ctypes.c_float * 3)()
            st = L.tsamd_spmm_profiled(*args, ms)
            profile[:] = [float(ms[0]), float(ms[1]), float(ms[2])]
    check(st, 'tsamd_spmm')
    return out, arg


SPMM_ROUTE_FIELDS = ('family', 'vec', 'slots', 'lpr', 'lgG', 'ktiles', 'P', 'items', 'snap', 'relabel', 'copy', 'fixup',
                     'table_off', 'tail_row_off', 'head_row_off', 'relabel_flag_off', 'records', 'grid_y',
                     'workspace_bytes')
SPMM_FAMILIES = ('none', 'short', 'cooperative', 'hot_rows', 'hot_blocks', 'arg32_short', 'arg32_cooperative',
                 'reference_order')


def spmm_route(dtype, reduce, B, M, N, K, E, mat=0, out=0, arg_out=0, arg32=False, workspace=0):
    """C-ABI ``tsamd_spmm_route`` (host arithmetic, no device): what the forward decides for these operands, as a dict of
    SPMM_ROUTE_FIELDS (``family`` as one of SPMM_FAMILIES).  mat / out / arg_out / workspace: tensors or plain addresses
    (they count for their alignment and the offsets only; 0 = aligned / no workspace).  A refusal raises TsamdError."""
    def addr(p):
        return ctypes.c_void_p(int(p.data_ptr() if hasattr(p, 'data_ptr') else p))
    words = (ctypes.c_int64 * 24)()
    st = lib().tsamd_spmm_route(dtype_code(dtype), REDUCES[reduce], _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), addr(mat),
                                addr(out), addr(arg_out), ctypes.c_int(1 if arg32 else 0), addr(workspace), words)
    check(st, 'tsamd_spmm_route')
    r = dict(zip(SPMM_ROUTE_FIELDS, (int(x) for x in words)))
    r['family'] = SPMM_FAMILIES[r['family']]
    return r


SPMM_ORDER_FIELDS = ('hdr_off', 'order_off', 'P', 'keys_off', 'shift', 'min_singles', 'bucket_max')


def spmm_order_layout(dtype, reduce, B, M, N, K, E, mat, out, workspace):
    """C-ABI ``tsamd_spmm_order_layout`` (host arithmetic): None when the call keeps slot = partition, else a dict of
    SPMM_ORDER_FIELDS plus ``mode`` (1 auto, 2 forced).  mat / out / workspace: tensors or plain addresses."""
    def addr(p):
        return ctypes.c_void_p(int(p.data_ptr() if hasattr(p, 'data_ptr') else p))
    words = (ctypes.c_int64 * 8)()
    mode = lib().tsamd_spmm_order_layout(dtype_code(dtype), REDUCES[reduce], _i64(B), _i64(M), _i64(N), _i64(K), _i64(E),
                                         addr(mat), addr(out), addr(workspace), words)
    if mode == 0:
        return None
    r = dict(zip(SPMM_ORDER_FIELDS, (int(x) for x in words)))
    r['mode'] = int(mode)
    return r


SPMM_HINTS_FIELDS = ('flags_off', 'hdr_off', 'totals_off', 'words_off', 'lists_off', 'order_off', 'P', 'bytes')


def spmm_hints_bytes(dtype, reduce, B, M, N, K, E):
    """C-ABI ``tsamd_spmm_hints_bytes``: the size of a pattern's hints buffer, 0 when the call is out of scope."""
    return int(lib().tsamd_spmm_hints_bytes(dtype_code(dtype), REDUCES[reduce], _i64(B), _i64(M), _i64(N), _i64(K), _i64(E)))


def spmm_hints_layout(dtype, reduce, B, M, N, K, E):
    """C-ABI ``tsamd_spmm_hints_layout`` (host arithmetic): None when the call is out of scope, else a dict of
    SPMM_HINTS_FIELDS."""
    words = (ctypes.c_int64 * 8)()
    if lib().tsamd_spmm_hints_layout(dtype_code(dtype), REDUCES[reduce], _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), words) == 0:
        return None
    return dict(zip(SPMM_HINTS_FIELDS, (int(x) for x in words)))


def spmm_hinted(rowptr, col, value, mat, reduce, hints, state, ws=None):
    """C-ABI ``tsamd_spmm_hinted`` on one [N, K] matrix: ``hints`` a uint8 device tensor of ``spmm_hints_bytes``,
    ``state`` 1 builds it, 2 reuses it.  Returns out."""
    require_gpu(rowptr, col, value, mat, hints)
    red, dt = REDUCES[reduce], dtype_code(mat.dtype)
    M, E, N, K = rowptr.numel() - 1, col.numel(), mat.size(0), mat.size(1)
    out = torch.empty((M, K), dtype=mat.dtype, device=mat.device)
    L = lib()
    if ws is None:
        ws = workspace(L.tsamd_spmm_workspace_bytes(dt, red, _i64(1), _i64(M), _i64(N), _i64(K), _i64(E)), mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_hinted(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(None), _i64(1),
                                 _i64(M), _i64(N), _i64(K), _i64(E), _ptr(ws), ctypes.c_size_t(ws.numel()), _ptr(hints),
                                 ctypes.c_int(int(state)), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_hinted')
    return out


def spmm_partial(rowptr, col, value, mat, reduce, out, arg_out=None, arg_map=None, arg_none=0, accumulate=True,
                 deg_rowptr=None):
    """C-ABI ``tsamd_spmm_partial``: the product of one column block combined into ``out`` / ``arg_out`` in place
    (``accumulate=False``: the first block overwrites them).  mat: [N, K] or [B, N, K] contiguous."""
    require_gpu(rowptr, col, value, mat, out, arg_out, arg_map, deg_rowptr)
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    if value is not None and value.dtype != mat.dtype:
        raise TsamdError('expected scalar type %s but found %s' % (mat.dtype, value.dtype))
    if not (mat.is_contiguous() and out.is_contiguous() and (arg_out is None or arg_out.is_contiguous())):
        raise TsamdError('tsamd_spmm_partial works in place: mat / out / arg_out must be contiguous')
    if out.dtype != mat.dtype or (red >= 2 and (arg_out is None or arg_out.dtype != torch.int64)):
        raise TsamdError('Input mismatch: out / arg_out')
    M, E = rowptr.numel() - 1, col.numel()
    N, K = mat.size(-2), mat.size(-1)
    B = mat.numel() // max(N * K, 1) if N * K > 0 else 1
    if out.numel() != B * M * K or (arg_out is not None and arg_out.numel() != out.numel()):
        raise TsamdError('Input mismatch: out must be [B, M, K]')
    L = lib()
    nb = L.tsamd_spmm_partial_workspace_bytes(dt, red, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E))
    ws = workspace(nb, mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_partial(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(arg_out),
                                  _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), _ptr(arg_map), _i64(arg_none),
                                  ctypes.c_int(1 if accumulate else 0), _ptr(deg_rowptr), _ptr(ws),
                                  ctypes.c_size_t(ws.numel()), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_partial')
    return out, arg_out


def spmm_value_bw(row, rowptr, col, mat, grad, reduce):
    """C-ABI ``tsamd_spmm_value_bw``: gradient w.r.t. the sparse values, [E]."""
    require_gpu(rowptr, col, mat, grad, row)
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    mat, grad = mat.contiguous(), grad.contiguous()
    if grad.dtype != mat.dtype:
        raise TsamdError('expected scalar type %s but found %s' % (mat.dtype, grad.dtype))
    M, E = rowptr.numel() - 1, col.numel()
    N, K = mat.size(-2), mat.size(-1)
    B = mat.numel() // (N * K) if N * K > 0 else 1
    out = torch.empty(E, dtype=mat.dtype, device=mat.device)
    with torch.cuda.device(mat.device):
        st = lib().tsamd_spmm_value_bw(dt, red, _ptr(row), _ptr(rowptr), _ptr(col), _ptr(mat),
                                       _ptr(grad), _ptr(out), _i64(B), _i64(M), _i64(N), _i64(K),
                                       _i64(E), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_value_bw')
    return out


def spspmm_bw_route(dtype):
    """C-ABI ``tsamd_spspmm_bw_route`` (host arithmetic, no device): the eight route words for a value dtype."""
    out = (ctypes.c_int64 * 8)()
    check(lib().tsamd_spspmm_bw_route(dtype_code(dtype), out), 'tsamd_spspmm_bw_route')
    return [int(x) for x in out]


def spspmm_value_bw(side, segptr, segind, listptr, list_ind, list_val, rowptrC, colC, gC, grad=None):
    """C-ABI ``tsamd_spspmm_bw_plan`` + ``tsamd_spspmm_value_bw``: the gradient of one value tensor of C = A * B.
    side 0 (gA): (rowptrA, colA, rowptrB, colB, valB or None); side 1 (gB): (rowptrB, colB, colptrA, rowA and valA
    in column order, or None).  grad: an optional contiguous [nseg] buffer to write into.  Returns (grad [nseg], P); one
    host sync (the plan's stats)."""
    require_gpu(segptr, segind, listptr, list_ind, list_val, rowptrC, colC, gC)
    if list_val is not None and list_val.dtype != gC.dtype:
        raise TsamdError('expected scalar type %s but found %s' % (gC.dtype, list_val.dtype))
    if not gC.is_contiguous() or (list_val is not None and not list_val.is_contiguous()):
        raise TsamdError('tsamd_spspmm_value_bw: gC / list_val must be contiguous')
    dev = gC.device
    dt = dtype_code(gC.dtype)
    nrows, nseg = segptr.numel() - 1, segind.numel()
    L = lib()
    ptr = torch.empty(nseg + 1, dtype=torch.int64, device=dev)
    stats = torch.empty(2, dtype=torch.int64, device=dev)
    if grad is None:
        grad = torch.empty(nseg, dtype=gC.dtype, device=dev)
    elif grad.dtype != gC.dtype or grad.numel() != nseg or not grad.is_contiguous() or grad.device != dev:
        raise TsamdError('tsamd_spspmm_value_bw: grad must be a contiguous [nseg] tensor of the type of gC')
    ws0 = workspace(L.tsamd_spspmm_bw_plan_workspace_bytes(_i64(nseg)), dev)
    with torch.cuda.device(dev):
        st = L.tsamd_spspmm_bw_plan(dt, ctypes.c_int(side), _ptr(segptr), _i64(nrows), _ptr(segind), _i64(nseg),
                                    _ptr(listptr), _ptr(ptr), _ptr(stats), _ptr(ws0), ctypes.c_size_t(ws0.numel()),
                                    stream_ptr(dev))
        check(st, 'tsamd_spspmm_bw_plan')
        nbytes, P = (int(x) for x in stats.cpu())
        assert nbytes == L.tsamd_spspmm_bw_workspace_bytes(dt, _i64(P))
        ws = workspace(nbytes, dev)
        st = L.tsamd_spspmm_value_bw(dt, ctypes.c_int(side), _ptr(ptr), _i64(P), _ptr(segptr), _i64(nrows),
                                     _ptr(segind), _i64(nseg), _ptr(listptr), _ptr(list_ind), _ptr(list_val),
                                     _ptr(rowptrC), _ptr(colC), _ptr(gC), _ptr(grad), _ptr(ws),
                                     ctypes.c_size_t(ws.numel()), stream_ptr(dev))
    check(st, 'tsamd_spspmm_value_bw')
    return grad, P


def _given(buf, numel, dtype, what):
    """A caller's output buffer (tests fill it with a sentinel first): contiguous, of the right type and size."""
    if buf.dtype != dtype or buf.numel() != numel or not buf.is_contiguous():
        raise TsamdError('%s: the given buffer must be contiguous, %s, %d elements' % (what, dtype, numel))
    return buf


def _out_buffer(given, wanted, numel, mat, like=False):
    if not wanted:
        return None
    if given is not None:
        return _given(given, numel, mat.dtype, 'output')
    return torch.empty_like(mat) if like else torch.empty(numel, dtype=mat.dtype, device=mat.device)


MINMAX_BW_ROUTE_FIELDS = ('status', 'value', 'sddmm', 'sddmm_lgG', 'mat', 'write_records', 'W', 'S', 'has_z', 'lgG', 'cap',
                          'packed', 'shadow', 'shadow_bytes', 'items', 'P', 'fixup', 'relabel', 'copy', 'vec', 'lpr',
                          'sum_lgG', 'ktiles', 'workspace_bytes', 'family')
MINMAX_BW_WINNERS = ('ids64', 'ids32', 'records', 'none')
MINMAX_BW_VALUE = ('none', 'zero', 'masked_sddmm', 'row_parallel')
MINMAX_BW_SDDMM = ('none', 'pipelined', 'round4')
MINMAX_BW_MAT = ('none', 'zero', 'pull', 'scatter')
MINMAX_BW_PACKED = ('plain', 'merge_pairs', 'idx_parity')


def spmm_minmax_bw_route(winners, dtype, B, M, N, K, E, want_value=False, want_mat=True, mat=0, grad_out=0, grad_mat=0):
    """C-ABI ``tsamd_spmm_minmax_bw_route`` (host arithmetic, no device): what the min / max backward decides for these
    operands, as a dict of MINMAX_BW_ROUTE_FIELDS.  winners: one of MINMAX_BW_WINNERS ('none': the bare scatter entry);
    mat / grad_out / grad_mat: tensors or plain addresses (their alignment counts; 0 = aligned).  ``status`` is the
    entry's answer as an int (0 = OK; the other fields are then filled), ``value`` / ``sddmm`` / ``mat`` / ``packed`` are
    names, ``family`` one of SPMM_FAMILIES."""
    def addr(p):
        return ctypes.c_void_p(int(p.data_ptr() if hasattr(p, 'data_ptr') else p))
    words = (ctypes.c_int64 * 32)()
    dt = dtype if isinstance(dtype, int) else dtype_code(dtype)
    st = lib().tsamd_spmm_minmax_bw_route(MINMAX_BW_WINNERS.index(winners), dt, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E),
                                          ctypes.c_int(1 if want_value else 0), ctypes.c_int(1 if want_mat else 0),
                                          addr(mat), addr(grad_out), addr(grad_mat), words)
    check(st, 'tsamd_spmm_minmax_bw_route')
    r = dict(zip(MINMAX_BW_ROUTE_FIELDS, (int(x) for x in words)))
    r['value'] = MINMAX_BW_VALUE[r['value']]
    r['sddmm'] = MINMAX_BW_SDDMM[r['sddmm']]
    r['mat'] = MINMAX_BW_MAT[r['mat']]
    r['packed'] = MINMAX_BW_PACKED[r['packed']]
    r['family'] = SPMM_FAMILIES[r['family']]
    return r


def spmm_minmax_bw(rowptr, col, value, mat, grad_out, arg_out, want_value=True, want_mat=True, gv=None, gm=None):
    """C-ABI ``tsamd_spmm_minmax_bw``: (grad_value or None, grad_mat or None).  ``rowptr`` may be
    None when ``want_value`` is False.  gv / gm: buffers to write into instead of fresh ones."""
    require_gpu(rowptr, col, value, mat, grad_out, arg_out)
    dt = dtype_code(mat.dtype)
    mat, grad_out, arg_out = mat.contiguous(), grad_out.contiguous(), arg_out.contiguous()
    E = col.numel()
    N, K = mat.size(-2), mat.size(-1)
    M = grad_out.size(-2)
    B = mat.numel() // (N * K) if N * K > 0 else 1
    gv = _out_buffer(gv, want_value, E, mat)
    gm = _out_buffer(gm, want_mat, mat.numel(), mat, like=True)
    L = lib()
    nb = L.tsamd_spmm_minmax_bw_workspace_bytes(dt, _i64(B), _i64(N), _i64(K), _i64(E))
    if gm is not None and gm.data_ptr() % 4 != 0:  # a misaligned f16 / bf16 grad_mat takes the fp32 shadow at any count
        nb = max(nb, 4 * B * N * K + 256)
    ws = workspace(nb, mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_bw(dt, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(grad_out),
                                    _ptr(arg_out), _ptr(gv), _ptr(gm), _i64(B), _i64(M), _i64(N),
                                    _i64(K), _i64(E), _ptr(ws), ctypes.c_size_t(ws.numel()),
                                    stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_bw')
    return gv, gm


def spmm_minmax_arg32(rowptr, col, value, mat, reduce):
    """C-ABI ``tsamd_spmm_minmax_arg32`` (stateless): min / max with the winners as int32 ids -> (out, arg32)."""
    require_gpu(rowptr, col, value, mat)
    mat = mat.contiguous()
    M, E = rowptr.numel() - 1, col.numel()
    N, K = mat.size(-2), mat.size(-1)
    B = mat.numel() // (N * K) if N * K > 0 else 1
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    out = torch.empty(list(mat.shape[:-2]) + [M, K], dtype=mat.dtype, device=mat.device)
    arg = torch.empty(out.shape, dtype=torch.int32, device=mat.device)
    L = lib()
    nbytes = L.tsamd_spmm_workspace_bytes(dt, red, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E))
    ws = workspace(nbytes, mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_arg32(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(arg),
                                       _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), _ptr(ws),
                                       ctypes.c_size_t(ws.numel()), None, ctypes.c_size_t(0), 0,
                                       stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_arg32')
    return out, arg


def spmm_minmax_bw_csc(rowptr, col, value, mat, grad_out, arg_out, colptr, csr2csc, row, want_value=True,
                       want_mat=True, gv=None, gm=None):
    """C-ABI ``tsamd_spmm_minmax_bw_csc`` (pull formulation over the CSC arrays, no atomics):
    (grad_value or None, grad_mat or None).  gv / gm: buffers to write into instead of fresh ones."""
    require_gpu(rowptr, col, value, mat, grad_out, arg_out, colptr, csr2csc, row)
    dt = dtype_code(mat.dtype)
    mat, grad_out, arg_out = mat.contiguous(), grad_out.contiguous(), arg_out.contiguous()
    E = col.numel()
    N, K = mat.size(-2), mat.size(-1)
    M = grad_out.size(-2)
    B = mat.numel() // (N * K) if N * K > 0 else 1
    gv = _out_buffer(gv, want_value, E, mat)
    gm = _out_buffer(gm, want_mat, mat.numel(), mat, like=True)
    L = lib()
    nb = L.tsamd_spmm_minmax_bw_csc_workspace_bytes(dt, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E))
    ws = workspace(nb, mat.device)
    fn = L.tsamd_spmm_minmax_bw_csc_arg32 if arg_out.dtype == torch.int32 else L.tsamd_spmm_minmax_bw_csc
    with torch.cuda.device(mat.device):
        st = fn(dt, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(grad_out),
                _ptr(arg_out), _ptr(colptr), _ptr(csr2csc), _ptr(row), _ptr(gv), _ptr(gm),
                _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), _ptr(ws),
                ctypes.c_size_t(ws.numel()), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_bw_csc')
    return gv, gm


def spmm_minmax_records(rowptr, col, value, mat, reduce, row, zero=False, out=None, rec=None):
    """C-ABI ``tsamd_spmm_minmax_records``: min / max forward that leaves the winner records of the pull backward
    -> (out, records as int32 words).  zero: the buffer starts as zeros (padding words of a record are never written)."""
    require_gpu(rowptr, col, value, mat, row)
    mat = mat.contiguous()
    M, E = rowptr.numel() - 1, col.numel()
    N, K = mat.size(-2), mat.size(-1)
    B = mat.numel() // (N * K) if N * K > 0 else 1
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    if out is None:
        out = torch.empty(list(mat.shape[:-2]) + [M, K], dtype=mat.dtype, device=mat.device)
    else:
        _given(out, B * M * K, mat.dtype, 'out')
    L = lib()
    nrec = L.tsamd_spmm_minmax_records_bytes(_i64(B), _i64(K), _i64(E)) // 4
    if rec is None:
        rec = (torch.zeros if zero else torch.empty)(nrec, dtype=torch.int32, device=mat.device)
    else:
        _given(rec, nrec, torch.int32, 'records')
    ws = workspace(L.tsamd_spmm_minmax_records_workspace_bytes(dt, red, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E)),
                   mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_records(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(row),
                                         _ptr(rec), _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), _ptr(ws),
                                         ctypes.c_size_t(ws.numel()), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_records')
    return out, rec


def spmm_minmax_winrec(row, value, arg32, K, rec=None, dtype=None):
    """C-ABI ``tsamd_spmm_minmax_winrec``: the winner records of int32 winner ids [B, M, K] -> int32 words."""
    require_gpu(row, value, arg32)
    arg32 = arg32.contiguous()
    E, M = row.numel(), arg32.size(-2)
    B = arg32.numel() // (M * K) if M * K > 0 else 1
    L = lib()
    nrec = L.tsamd_spmm_minmax_records_bytes(_i64(B), _i64(K), _i64(E)) // 4
    if rec is None:
        rec = torch.zeros(nrec, dtype=torch.int32, device=row.device)
    else:
        _given(rec, nrec, torch.int32, 'records')
    dt = dtype_code(value.dtype) if value is not None else (dtype_code(dtype) if dtype is not None else 0)
    with torch.cuda.device(row.device):
        st = L.tsamd_spmm_minmax_winrec(dt, _ptr(row), _ptr(value), _ptr(arg32), _ptr(rec), _i64(B), _i64(M), _i64(K),
                                        _i64(E), stream_ptr(row.device))
    check(st, 'tsamd_spmm_minmax_winrec')
    return rec


def spmm_minmax_bw_csc_records(rowptr, col, has_value, mat, grad_out, records, colptr, csr2csc, row, want_value=False,
                               gv=None, gm=None):
    """C-ABI ``tsamd_spmm_minmax_bw_csc_records``: the pull backward on records -> (grad_value or None, grad_mat)."""
    require_gpu(rowptr, col, mat, grad_out, records, colptr, csr2csc, row)
    dt = dtype_code(mat.dtype)
    mat, grad_out = mat.contiguous(), grad_out.contiguous()
    E = col.numel()
    N, K = mat.size(-2), mat.size(-1)
    M = grad_out.size(-2)
    B = mat.numel() // (N * K) if N * K > 0 else 1
    gv = _out_buffer(gv, want_value, E, mat)
    gm = _out_buffer(gm, True, mat.numel(), mat, like=True)
    L = lib()
    ws = workspace(L.tsamd_spmm_minmax_bw_csc_records_workspace_bytes(dt, _i64(B), _i64(M), _i64(N), _i64(K), _i64(E)),
                   mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_bw_csc_records(dt, _ptr(rowptr), _ptr(col), ctypes.c_int(1 if has_value else 0), _ptr(mat),
                                                _ptr(grad_out), _ptr(records), _ptr(colptr), _ptr(csr2csc), _ptr(row),
                                                _ptr(gv), _ptr(gm), _i64(B), _i64(M), _i64(N), _i64(K), _i64(E), _ptr(ws),
                                                ctypes.c_size_t(ws.numel()), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_bw_csc_records')
    return gv, gm


def ind2ptr(ind, M):
    require_gpu(ind)
    out = torch.empty(M + 1, dtype=torch.int64, device=ind.device)
    with torch.cuda.device(ind.device):
        st = lib().tsamd_ind2ptr(_ptr(ind), _i64(M), _i64(ind.numel()), _ptr(out),
                                 stream_ptr(ind.device))
    check(st, 'tsamd_ind2ptr')
    return out


def ptr2ind(ptr, E):
    require_gpu(ptr)
    out = torch.empty(E, dtype=torch.int64, device=ptr.device)
    with torch.cuda.device(ptr.device):
        st = lib().tsamd_ptr2ind(_ptr(ptr), _i64(ptr.numel() - 1), _i64(E), _ptr(out),
                                 stream_ptr(ptr.device))
    check(st, 'tsamd_ptr2ind')
    return out
