"""ctypes binding of the C-ABI in ``include/tsamd.h`` (``lib/libtsamd.so``).

This is the thin layer that hands torch device pointers, sizes and the current
HIP stream to the hand-written kernels.  There is no CPU implementation behind
it: a missing library, a CPU tensor or a non-zero status raises.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TSAMD_LIB') or os.path.join(_HERE, 'lib', 'libtsamd.so')

# the header the signatures are read from: $TSAMD_HEADER, else the copy an installed package carries, else the tree's
_SHIPPED = os.path.join(_HERE, 'include', 'tsamd.h')
HEADER_PATH = os.environ.get('TSAMD_HEADER') or (
    _SHIPPED if os.path.exists(_SHIPPED) else os.path.join(os.path.dirname(_HERE), 'include', 'tsamd.h'))

_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'uint32_t': ctypes.c_uint32,
            'size_t': ctypes.c_size_t, 'double': ctypes.c_double, 'float': ctypes.c_float}
_PROTOTYPE = re.compile(r'([\w\s*]+?)\b(tsamd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;')


def _ctype(decl, name, param):
    """The ctypes type of one parameter declaration (with or without its name) or of a return type."""
    words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
    if param:
        if '*' in words or decl.rstrip().endswith(']'):
            return ctypes.c_void_p  # takes ints, None, c_void_p, ctypes arrays and pointers, byref()
        words = words[:-1] or words  # drop the parameter's name
    elif words in (['void'], ['char', '*']):
        return None if words == ['void'] else ctypes.c_char_p
    if len(words) != 1 or words[0] not in _SCALARS:
        raise TypeError('include/tsamd.h: %s: no ctypes mapping for `%s`' % (name, ' '.join(decl.split())))
    return _SCALARS[words[0]]


def parse_header(text):
    """{name: (restype, [argtypes])} for every ``ret tsamd_name(params);`` of the header's text.  A type outside the
    table above and a prototype this does not read (one that is not in that plain form) both raise."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*|^[ \t]*#[^\n]*', ' ', text, flags=re.M)
    table = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = [] if params.strip() == 'void' else params.split(',')
        table[name] = (_ctype(ret, name, False), [_ctype(p, name, True) for p in params])
    unread = set(re.findall(r'\b(tsamd_[a-z0-9_]+)\s*\(', text)) - set(table)
    if unread:
        raise TypeError('include/tsamd.h: prototype(s) not in the plain form the binding reads: %s' % sorted(unread))
    return table


def load_signatures():
    """The signature table of the header at HEADER_PATH; a missing header is as fatal as a missing library."""
    if not os.path.exists(HEADER_PATH):
        raise ImportError(
            'pytorch_sparse_amd: %s is missing. The ctypes binding takes every signature from this header '
            '(TSAMD_HEADER names another place). There is no CPU fallback.' % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


SIGNATURES = load_signatures()
SYMBOLS = sorted(SIGNATURES)  # every symbol include/tsamd.h declares (tests check that all of them resolve)

DTYPES = {
    torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3,
    torch.int32: 4, torch.int64: 5, torch.uint8: 6, torch.int8: 7, torch.int16: 8,
}
REDUCES = {'sum': 0, 'add': 0, 'mean': 1, 'min': 2, 'max': 3}

_lib = None


class TsamdError(RuntimeError):
    pass


def declare(L, names=SYMBOLS):
    """Give these functions of a loaded library the restype and argtypes the header states."""
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return L


def lib():
    """Load libtsamd.so once, every function declared as in the header; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                'pytorch_sparse_amd: %s is missing. Build it with '
                '`python pytorch_sparse_amd/build.py` (needs hipcc, targets gfx950). '
                'There is no CPU fallback.' % LIB_PATH)
        _lib = declare(ctypes.CDLL(LIB_PATH))
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


def _addr(p):
    """A tensor or a plain address, as an address."""
    return int(p.data_ptr() if hasattr(p, 'data_ptr') else p)


def _dims(M, col, mat):
    """(B, M, N, K, E) of a product with ``mat`` [..., N, K]; an empty matrix counts as one batch."""
    N, K = mat.size(-2), mat.size(-1)
    return (mat.numel() // (N * K) if N * K > 0 else 1), M, N, K, col.numel()


def _i64(x):
    """For raw calls in tests; the wrappers below pass plain ints (a c_int64 satisfies an int64_t parameter)."""
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
    B, M, N, K, E = _dims(rowptr.numel() - 1, col, mat)
    sizes = list(mat.shape)
    sizes[-2] = M
    if out is None:
        out = torch.empty(sizes, dtype=mat.dtype, device=mat.device)
    arg = None
    if red >= 2:
        arg = torch.empty(sizes, dtype=torch.int64, device=mat.device)
    L = lib()
    nb = L.tsamd_spmm_workspace_bytes(dt, red, B, M, N, K, E)
    ws = workspace(nb, mat.device)
    with torch.cuda.device(mat.device):
        args = (dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(arg),
                B, M, N, K, E, _ptr(ws), ws.numel(), stream_ptr(mat.device))
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
    words = (ctypes.c_int64 * 24)()
    st = lib().tsamd_spmm_route(dtype_code(dtype), REDUCES[reduce], B, M, N, K, E, _addr(mat), _addr(out), _addr(arg_out),
                                1 if arg32 else 0, _addr(workspace), words)
    check(st, 'tsamd_spmm_route')
    r = dict(zip(SPMM_ROUTE_FIELDS, (int(x) for x in words)))
    r['family'] = SPMM_FAMILIES[r['family']]
    return r


SPMM_ORDER_FIELDS = ('hdr_off', 'order_off', 'P', 'keys_off', 'shift', 'min_singles', 'bucket_max')


def spmm_order_layout(dtype, reduce, B, M, N, K, E, mat, out, workspace):
    """C-ABI ``tsamd_spmm_order_layout`` (host arithmetic): None when the call keeps slot = partition, else a dict of
    SPMM_ORDER_FIELDS plus ``mode`` (1 auto, 2 forced).  mat / out / workspace: tensors or plain addresses."""
    words = (ctypes.c_int64 * 8)()
    mode = lib().tsamd_spmm_order_layout(dtype_code(dtype), REDUCES[reduce], B, M, N, K, E, _addr(mat), _addr(out),
                                         _addr(workspace), words)
    if mode == 0:
        return None
    r = dict(zip(SPMM_ORDER_FIELDS, (int(x) for x in words)))
    r['mode'] = int(mode)
    return r


SPMM_HINTS_FIELDS = ('flags_off', 'hdr_off', 'totals_off', 'words_off', 'lists_off', 'order_off', 'P', 'bytes')


def spmm_hints_bytes(dtype, reduce, B, M, N, K, E):
    """C-ABI ``tsamd_spmm_hints_bytes``: the size of a pattern's hints buffer, 0 when the call is out of scope."""
    return int(lib().tsamd_spmm_hints_bytes(dtype_code(dtype), REDUCES[reduce], B, M, N, K, E))


def spmm_hints_layout(dtype, reduce, B, M, N, K, E):
    """C-ABI ``tsamd_spmm_hints_layout`` (host arithmetic): None when the call is out of scope, else a dict of
    SPMM_HINTS_FIELDS."""
    words = (ctypes.c_int64 * 8)()
    if lib().tsamd_spmm_hints_layout(dtype_code(dtype), REDUCES[reduce], B, M, N, K, E, words) == 0:
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
        ws = workspace(L.tsamd_spmm_workspace_bytes(dt, red, 1, M, N, K, E), mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_hinted(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), None, 1, M, N, K, E,
                                 _ptr(ws), ws.numel(), _ptr(hints), int(state), stream_ptr(mat.device))
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
    B, M, N, K, E = _dims(rowptr.numel() - 1, col, mat)
    if out.numel() != B * M * K or (arg_out is not None and arg_out.numel() != out.numel()):
        raise TsamdError('Input mismatch: out must be [B, M, K]')
    L = lib()
    nb = L.tsamd_spmm_partial_workspace_bytes(dt, red, B, M, N, K, E)
    ws = workspace(nb, mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_partial(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(arg_out),
                                  B, M, N, K, E, _ptr(arg_map), int(arg_none), 1 if accumulate else 0, _ptr(deg_rowptr),
                                  _ptr(ws), ws.numel(), stream_ptr(mat.device))
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
    B, M, N, K, E = _dims(rowptr.numel() - 1, col, mat)
    out = torch.empty(E, dtype=mat.dtype, device=mat.device)
    with torch.cuda.device(mat.device):
        st = lib().tsamd_spmm_value_bw(dt, red, _ptr(row), _ptr(rowptr), _ptr(col), _ptr(mat), _ptr(grad), _ptr(out),
                                       B, M, N, K, E, stream_ptr(mat.device))
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
    ws0 = workspace(L.tsamd_spspmm_bw_plan_workspace_bytes(nseg), dev)
    with torch.cuda.device(dev):
        st = L.tsamd_spspmm_bw_plan(dt, side, _ptr(segptr), nrows, _ptr(segind), nseg, _ptr(listptr), _ptr(ptr),
                                    _ptr(stats), _ptr(ws0), ws0.numel(), stream_ptr(dev))
        check(st, 'tsamd_spspmm_bw_plan')
        nbytes, P = (int(x) for x in stats.cpu())
        assert nbytes == L.tsamd_spspmm_bw_workspace_bytes(dt, P)
        ws = workspace(nbytes, dev)
        st = L.tsamd_spspmm_value_bw(dt, side, _ptr(ptr), P, _ptr(segptr), nrows, _ptr(segind), nseg, _ptr(listptr),
                                     _ptr(list_ind), _ptr(list_val), _ptr(rowptrC), _ptr(colC), _ptr(gC), _ptr(grad),
                                     _ptr(ws), ws.numel(), stream_ptr(dev))
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
    words = (ctypes.c_int64 * 32)()
    dt = dtype if isinstance(dtype, int) else dtype_code(dtype)
    st = lib().tsamd_spmm_minmax_bw_route(MINMAX_BW_WINNERS.index(winners), dt, B, M, N, K, E, 1 if want_value else 0,
                                          1 if want_mat else 0, _addr(mat), _addr(grad_out), _addr(grad_mat), words)
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
    B, M, N, K, E = _dims(grad_out.size(-2), col, mat)
    gv = _out_buffer(gv, want_value, E, mat)
    gm = _out_buffer(gm, want_mat, mat.numel(), mat, like=True)
    L = lib()
    nb = L.tsamd_spmm_minmax_bw_workspace_bytes(dt, B, N, K, E)
    if gm is not None and gm.data_ptr() % 4 != 0:  # a misaligned f16 / bf16 grad_mat takes the fp32 shadow at any count
        nb = max(nb, 4 * B * N * K + 256)
    ws = workspace(nb, mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_bw(dt, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(grad_out),
                                    _ptr(arg_out), _ptr(gv), _ptr(gm), B, M, N, K, E, _ptr(ws), ws.numel(),
                                    stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_bw')
    return gv, gm


def spmm_minmax_arg32(rowptr, col, value, mat, reduce):
    """C-ABI ``tsamd_spmm_minmax_arg32`` (stateless): min / max with the winners as int32 ids -> (out, arg32)."""
    require_gpu(rowptr, col, value, mat)
    mat = mat.contiguous()
    B, M, N, K, E = _dims(rowptr.numel() - 1, col, mat)
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    out = torch.empty(list(mat.shape[:-2]) + [M, K], dtype=mat.dtype, device=mat.device)
    arg = torch.empty(out.shape, dtype=torch.int32, device=mat.device)
    L = lib()
    nbytes = L.tsamd_spmm_workspace_bytes(dt, red, B, M, N, K, E)
    ws = workspace(nbytes, mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_arg32(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(arg),
                                       B, M, N, K, E, _ptr(ws), ws.numel(), None, 0, 0, stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_arg32')
    return out, arg


def spmm_minmax_bw_csc(rowptr, col, value, mat, grad_out, arg_out, colptr, csr2csc, row, want_value=True,
                       want_mat=True, gv=None, gm=None):
    """C-ABI ``tsamd_spmm_minmax_bw_csc`` (pull formulation over the CSC arrays, no atomics):
    (grad_value or None, grad_mat or None).  gv / gm: buffers to write into instead of fresh ones."""
    require_gpu(rowptr, col, value, mat, grad_out, arg_out, colptr, csr2csc, row)
    dt = dtype_code(mat.dtype)
    mat, grad_out, arg_out = mat.contiguous(), grad_out.contiguous(), arg_out.contiguous()
    B, M, N, K, E = _dims(grad_out.size(-2), col, mat)
    gv = _out_buffer(gv, want_value, E, mat)
    gm = _out_buffer(gm, want_mat, mat.numel(), mat, like=True)
    L = lib()
    nb = L.tsamd_spmm_minmax_bw_csc_workspace_bytes(dt, B, M, N, K, E)
    ws = workspace(nb, mat.device)
    fn = L.tsamd_spmm_minmax_bw_csc_arg32 if arg_out.dtype == torch.int32 else L.tsamd_spmm_minmax_bw_csc
    with torch.cuda.device(mat.device):
        st = fn(dt, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(grad_out), _ptr(arg_out), _ptr(colptr),
                _ptr(csr2csc), _ptr(row), _ptr(gv), _ptr(gm), B, M, N, K, E, _ptr(ws), ws.numel(), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_bw_csc')
    return gv, gm


def spmm_minmax_records(rowptr, col, value, mat, reduce, row, zero=False, out=None, rec=None):
    """C-ABI ``tsamd_spmm_minmax_records``: min / max forward that leaves the winner records of the pull backward
    -> (out, records as int32 words).  zero: the buffer starts as zeros (padding words of a record are never written)."""
    require_gpu(rowptr, col, value, mat, row)
    mat = mat.contiguous()
    B, M, N, K, E = _dims(rowptr.numel() - 1, col, mat)
    red = REDUCES[reduce]
    dt = dtype_code(mat.dtype)
    if out is None:
        out = torch.empty(list(mat.shape[:-2]) + [M, K], dtype=mat.dtype, device=mat.device)
    else:
        _given(out, B * M * K, mat.dtype, 'out')
    L = lib()
    nrec = L.tsamd_spmm_minmax_records_bytes(B, K, E) // 4
    if rec is None:
        rec = (torch.zeros if zero else torch.empty)(nrec, dtype=torch.int32, device=mat.device)
    else:
        _given(rec, nrec, torch.int32, 'records')
    ws = workspace(L.tsamd_spmm_minmax_records_workspace_bytes(dt, red, B, M, N, K, E), mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_records(dt, red, _ptr(rowptr), _ptr(col), _ptr(value), _ptr(mat), _ptr(out), _ptr(row),
                                         _ptr(rec), B, M, N, K, E, _ptr(ws), ws.numel(), stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_records')
    return out, rec


def spmm_minmax_winrec(row, value, arg32, K, rec=None, dtype=None):
    """C-ABI ``tsamd_spmm_minmax_winrec``: the winner records of int32 winner ids [B, M, K] -> int32 words."""
    require_gpu(row, value, arg32)
    arg32 = arg32.contiguous()
    E, M = row.numel(), arg32.size(-2)
    B = arg32.numel() // (M * K) if M * K > 0 else 1
    L = lib()
    nrec = L.tsamd_spmm_minmax_records_bytes(B, K, E) // 4
    if rec is None:
        rec = torch.zeros(nrec, dtype=torch.int32, device=row.device)
    else:
        _given(rec, nrec, torch.int32, 'records')
    dt = dtype_code(value.dtype) if value is not None else (dtype_code(dtype) if dtype is not None else 0)
    with torch.cuda.device(row.device):
        st = L.tsamd_spmm_minmax_winrec(dt, _ptr(row), _ptr(value), _ptr(arg32), _ptr(rec), B, M, K, E,
                                        stream_ptr(row.device))
    check(st, 'tsamd_spmm_minmax_winrec')
    return rec


def spmm_minmax_bw_csc_records(rowptr, col, has_value, mat, grad_out, records, colptr, csr2csc, row, want_value=False,
                               gv=None, gm=None):
    """C-ABI ``tsamd_spmm_minmax_bw_csc_records``: the pull backward on records -> (grad_value or None, grad_mat)."""
    require_gpu(rowptr, col, mat, grad_out, records, colptr, csr2csc, row)
    dt = dtype_code(mat.dtype)
    mat, grad_out = mat.contiguous(), grad_out.contiguous()
    B, M, N, K, E = _dims(grad_out.size(-2), col, mat)
    gv = _out_buffer(gv, want_value, E, mat)
    gm = _out_buffer(gm, True, mat.numel(), mat, like=True)
    L = lib()
    ws = workspace(L.tsamd_spmm_minmax_bw_csc_records_workspace_bytes(dt, B, M, N, K, E), mat.device)
    with torch.cuda.device(mat.device):
        st = L.tsamd_spmm_minmax_bw_csc_records(dt, _ptr(rowptr), _ptr(col), 1 if has_value else 0, _ptr(mat),
                                                _ptr(grad_out), _ptr(records), _ptr(colptr), _ptr(csr2csc), _ptr(row),
                                                _ptr(gv), _ptr(gm), B, M, N, K, E, _ptr(ws), ws.numel(),
                                                stream_ptr(mat.device))
    check(st, 'tsamd_spmm_minmax_bw_csc_records')
    return gv, gm


def ind2ptr(ind, M):
    require_gpu(ind)
    out = torch.empty(M + 1, dtype=torch.int64, device=ind.device)
    with torch.cuda.device(ind.device):
        st = lib().tsamd_ind2ptr(_ptr(ind), M, ind.numel(), _ptr(out), stream_ptr(ind.device))
    check(st, 'tsamd_ind2ptr')
    return out


def ptr2ind(ptr, E):
    require_gpu(ptr)
    out = torch.empty(E, dtype=torch.int64, device=ptr.device)
    with torch.cuda.device(ptr.device):
        st = lib().tsamd_ptr2ind(_ptr(ptr), ptr.numel() - 1, E, _ptr(out), stream_ptr(ptr.device))
    check(st, 'tsamd_ptr2ind')
    return out
