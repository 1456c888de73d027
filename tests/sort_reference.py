"""What the device-side route of the sort (csrc/sort.hip) depends on, restated in numpy, and a ctypes harness that lets
a test read the device's decision from a workspace it owns.  Importing this needs no GPU.

  bucket_ids   the bucket id sort_build_kernel histograms (and bucket_scatter_kernel recomputes), in the kernels' own
               arithmetic: 64-bit words that wrap, truncated to 32 bits
  fits         the predicate that keeps an entry on the bucket path: both ids inside the bit width of their size
  cases        the census of device routes and the table of wild ids (data only)
  sort_call    tsamd_sort_coo_values (modes 0-3), tsamd_sort_coalesce, tsamd_sort_coalesce_reduce with every output and
               the workspace between sentinel-filled guards, the workspace pre-filled with a sentinel byte

A "wild" id is one beyond the bit width of its size -- a row >= 2^bits_for(M), a col >= 2^bits_for(N), or a negative id
(read as unsigned).  An id that is merely out of range (row 300 .. 511 of M = 300) is not wild: its bucket id is an
ordinary one."""
import collections
import ctypes

import numpy as np

FIELDS = ('route', 'key_bits', 'idx_bits', 'packed', 'passes', 'ride', 'tiles',
          'on', 'levels', 'strip', 'bits', 'bits1', 'kshift', 'shift', 'nb', 'cap')
U64 = np.uint64


def bits_for(n):
    """Bits needed for ids in [0, n) (sort.hip: bits_for)."""
    b = 0
    while b < 63 and (1 << b) < n:
        b += 1
    return b


def route(E, M, N, value_bytes=0, coalesce=0):
    """The 16 fields of tsamd_sort_route as a dict, plus col_bits (not among them: the key layout's split)."""
    from pytorch_sparse_amd import _native as nat
    out = (ctypes.c_int64 * 16)()
    st = nat.lib().tsamd_sort_route(ctypes.c_int64(E), ctypes.c_int64(M), ctypes.c_int64(N), value_bytes, coalesce, out)
    assert st == 0, (E, M, N, value_bytes, coalesce, st)
    r = dict(zip(FIELDS, (int(x) for x in out)))
    r['col_bits'] = bits_for(max(N, 1))
    return r


def header(E, coalesce=0):
    """tsamd_sort_header: (byte offset of the header in the workspace, word of #descents, fast word, error word)."""
    from pytorch_sparse_amd import _native as nat
    out = (ctypes.c_int64 * 4)()
    st = nat.lib().tsamd_sort_header(ctypes.c_int64(E), coalesce, out)
    assert st == 0, (E, coalesce, st)
    return tuple(int(x) for x in out)


def _keys(row, col, route):
    r = np.asarray(row, dtype=np.int64).astype(U64)  # (two's complement: a negative id reads as huge)
    c = np.asarray(col, dtype=np.int64).astype(U64)
    return (r << U64(route['col_bits'])) | c         # wraps modulo 2^64, as the kernel's shift does


def bucket_ids(row, col, E, route, kernel='build'):
    """The bucket id of every entry as the kernels compute it WITHOUT looking at `fits` (int64 array of values below
    2^32).  kernel = 'build': sort_build_kernel; 'scatter': bucket_scatter_kernel level 1, which starts from the built
    word (a packed word has lost the key's top bits) and, in strip mode, from (key << 13 | place in the tile)."""
    assert route['on'] == 1
    key = _keys(row, col, route)
    i = np.arange(E, dtype=U64)
    idx_bits, packed = U64(route['idx_bits']), route['packed']
    if kernel == 'scatter':
        word = ((key << idx_bits) | i) if packed else key
        if route['strip']:
            k = (word >> idx_bits) if packed else word
            b = ((k << U64(13)) >> U64(13)) >> U64(route['key_bits'] - route['bits1'])
        else:
            b = word >> U64(route['shift'])
    elif route['strip']:
        b = key >> U64(route['kshift'])
    else:
        b = ((key << idx_bits) | i) >> U64(route['shift'])
    return (b & U64(0xffffffff)).astype(np.int64)


def pass_digits(row, col, E, route, kernel='pass'):
    """[passes, E] 8-bit digits of the one-sweep passes.  kernel = 'pass': what onesweep_pass_kernel reads from the
    built word; 'build': what sort_build_kernel histograms (the same bits of the same word); 'build_full_key': the
    digits of the whole 64-bit key, which a packed word cannot hold above bit 64 - idx_bits -- a histogram taken from
    these hands the passes runs of the wrong sizes as soon as a wild id sets such a bit."""
    key = _keys(row, col, route)
    idx_bits, packed = U64(route['idx_bits']), route['packed']
    out = np.empty((route['passes'], E), dtype=np.int64)
    for p in range(route['passes']):
        if kernel == 'pass':
            word = ((key << idx_bits) | np.arange(E, dtype=U64)) if packed else key
            d = word >> U64(8 * p + (route['idx_bits'] if packed else 0))
        elif kernel == 'build':
            d = (((key << idx_bits) >> idx_bits) if packed else key) >> U64(8 * p)
        else:
            assert kernel == 'build_full_key'
            d = key >> U64(8 * p)
        out[p] = (d & U64(255)).astype(np.int64)
    return out


def fits(row, col, route):
    """True where both ids lie inside their bit widths (the build kernel counts exactly these entries; any other entry
    takes the bucket path away from the whole input)."""
    r = np.asarray(row, dtype=np.int64).astype(U64)
    c = np.asarray(col, dtype=np.int64).astype(U64)
    row_bits = route['key_bits'] - route['col_bits']
    return ((r >> U64(row_bits)) | (c >> U64(route['col_bits']))) == U64(0)


# ---- the case tables ----
Case = collections.namedtuple('Case', 'name E M N kind fast on')
# census of device routes on in-range ids: the expected fast word of a sort that orders (see expected_fast)
CENSUS = (
    Case('full_131072', 131072, 300, 500, 'uniform', 1, 1),       # bucket path, full words: the first E with a plan
    Case('full_131073', 131073, 300, 500, 'uniform', 1, 1),       # ... one entry in the last scatter tile position
    Case('full_wide_131072', 131072, 9000, 7000, 'uniform', 1, 1),
    Case('full_wide_131073', 131073, 9000, 7000, 'uniform', 1, 1),
    Case('strip', (1 << 20) + 1, 1 << 22, 1 << 22, 'uniform', 1, 1),   # 44 + 21 bits: pairs, keys stripped of the bucket bits
    Case('posbits', 1 << 20, 16, 16, 'uniform', 1, 1),            # the bucket id reaches down to the position bits
    Case('hub', 500000, 1 << 20, 1 << 20, 'hub', 0, 1),           # a third of the entries in one row: a bucket overflows
    Case('sorted', 131072, 300, 500, 'sorted', 0, 1),             # no descents (with duplicates): copy + identity
    Case('below', 131071, 300, 500, 'uniform', 0, 0),             # below the threshold: no plan at all
)
RANKED = ('full_131073', 'strip')  # run under both rankings


def census():
    return CENSUS


def expected_fast(case, mode):
    """The fast word a sort of `case` through tsamd_sort_coo_values mode `mode` must leave (the probing sorts of the
    compacting entry points: mode 1).  A sorted input is ordered by the bucket path only when nobody probes (mode 0)."""
    if case.kind == 'sorted':
        return 1 if mode == 0 else 0
    return case.fast


def make_input(case, seed=None):
    """(row, col) int64 arrays: uniform ids with duplicates (stability shows in the permutation), a hub row, or sorted."""
    rng = np.random.default_rng(case.E % 1009 if seed is None else seed)
    row = rng.integers(0, case.M, case.E, dtype=np.int64)
    col = rng.integers(0, case.N, case.E, dtype=np.int64)
    if case.kind == 'hub':
        row[rng.permutation(case.E)[:case.E // 3]] = 12345
    q = case.E // 5
    row[:q], col[:q] = row[q:2 * q].copy(), col[q:2 * q].copy()
    if case.kind == 'sorted':
        perm = np.argsort(row * case.N + col, kind='stable')
        row, col = row[perm].copy(), col[perm].copy()
    return row, col


def reduce_runs(v_sorted, starts, op):
    """The fused reduction of the compacting bucket sort, bit for bit: every run of equal pairs reduced SEQUENTIALLY in
    sorted order in the element type (float32 / int32 accumulators; int32 mean = floor division) -- numpy's reduceat
    adds float32 pairwise, another association."""
    v = np.asarray(v_sorted)
    ends = np.append(starts[1:], v.size)
    length = ends - starts
    acc = v[starts].copy()
    with np.errstate(over='ignore'):
        for j in range(1, int(length.max())):
            has = length > j
            x = v[starts[has] + j]
            if op == 'min':
                acc[has] = np.where(x < acc[has], x, acc[has])
            elif op == 'max':
                acc[has] = np.where(x > acc[has], x, acc[has])
            else:
                acc[has] = acc[has] + x
    if op == 'mean':
        if np.issubdtype(v.dtype, np.integer):
            acc = np.floor_divide(acc, length.astype(v.dtype))
        else:
            acc = acc / length.astype(v.dtype)
    return acc.astype(v.dtype)


REDUCTIONS = ('sum', 'mean', 'min', 'max')

# wild ids: the two shapes, the kinds, where they are put
WILD_SHAPES = (
    Case('full', 131072, 300, 500, 'uniform', 0, 1),
    Case('strip', (1 << 20) + 1, 1 << 22, 1 << 22, 'uniform', 0, 1),
)
# one-sweep passes alone, packed words whose last digit reaches past bit 64 (47 + 17 bits, 6 passes of 8): a wild id
# sets key bits the word cannot hold -- the digit histogram must be taken from the word's bits
WILD_PASSES_ONLY = Case('passes_top_digit', 131071, 1 << 24, 1 << 23, 'uniform', 0, 0)


def wild_kinds(M, N):
    """(name, which, id).  'pow2' kinds: the first id beyond the bit width."""
    return (('row_pow2', 'row', 1 << bits_for(M)), ('row_2^40', 'row', 1 << 40), ('row_-1', 'row', -1),
            ('col_pow2', 'col', 1 << bits_for(N)), ('col_-5', 'col', -5), ('col_2^62', 'col', 1 << 62))


# Whether the id the kernels computed BEFORE the build kernel looked at `fits` lies outside the histogram (>= nb), by
# shape and kind -- from tests/test_sort_reference.py, no GPU run.  True: an index past the LDS histogram and the bucket
# offsets (the hazard).  False: the id wraps back below nb (bits shifted out of the 64-bit word, or a col bit that lands
# in the row bits of the key): no stray index, the entry only sorts under another key.
HAZARD = {
    ('full', 'row_pow2'): True, ('full', 'row_2^40'): False, ('full', 'row_-1'): True,
    ('full', 'col_pow2'): False, ('full', 'col_-5'): True, ('full', 'col_2^62'): False,
    ('strip', 'row_pow2'): True, ('strip', 'row_2^40'): True, ('strip', 'row_-1'): True,
    ('strip', 'col_pow2'): False, ('strip', 'col_-5'): True, ('strip', 'col_2^62'): True,
}


def wild_positions(E, where):
    """Entry positions that receive the wild id: first, last, the middle of a scatter tile (tiles of 256 x 30 or
    256 x 20 entries: position 3 * 7680 + 2560 is inside a tile for both), or 1 % of the entries."""
    if where == 'first':
        return np.array([0])
    if where == 'last':
        return np.array([E - 1])
    if where == 'mid_tile':
        return np.array([3 * 7680 + 2560])
    assert where == 'percent'
    return np.random.default_rng(7).permutation(E)[:E // 100]


WHERE = ('first', 'last', 'mid_tile', 'percent')


def cases():
    """The whole table as data: (census, wild shapes, wild kinds per shape, positions)."""
    return {'census': CENSUS, 'wild_shapes': WILD_SHAPES, 'where': WHERE, 'passes_only': WILD_PASSES_ONLY,
            'wild_kinds': {s.name: wild_kinds(s.M, s.N) for s in WILD_SHAPES}}


# ---- the harness ----
GUARD = 4096      # bytes on either side of every output and of the workspace
SENT = 0x5A       # the guards' and the untouched outputs' byte
WS_SENT = 0xA5    # what an earlier call "left" in the workspace


class Guarded:
    """`nbytes` of device memory between two GUARD-byte regions, everything filled with `fill`."""

    def __init__(self, nbytes, dev, fill=SENT):
        import torch
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD, ), fill, dtype=torch.uint8, device=dev)
        self.fill = fill
        self.ptr = ctypes.c_void_p(self.raw.data_ptr() + GUARD)

    def body(self, dtype=None):
        b = self.raw[GUARD:GUARD + self.nbytes]
        return b if dtype is None else b.view(dtype)

    def intact(self):
        return bool((self.raw[:GUARD] == self.fill).all()) and bool((self.raw[GUARD + self.nbytes:] == self.fill).all())

    def untouched(self):
        return bool((self.body() == self.fill).all())


Result = collections.namedtuple('Result', 'status out guards_ok hdr untouched ws')


def sort_call(entry, row, col, M, N, mode=0, counts_in=None, value=None, reduce=0, ws=None):
    """One call of a sort entry point on device tensors row / col (int64).

    entry: 'values' (tsamd_sort_coo_values, `mode` 0-3; mode 2 reads counts_in[0]), 'coalesce' (tsamd_sort_coalesce) or
    'reduce' (tsamd_sort_coalesce_reduce with `reduce` 0-3; value float32 / int32 or None).  value: a 1-D tensor of 4-
    or 8-byte elements, or None.  ws: the Guarded workspace of an earlier call to run on as it was left (dirty); else
    a fresh one filled with WS_SENT.
    -> Result(status, out = dict of output tensors (views into guarded storage), guards_ok, hdr = dict(descents, fast,
    error) read back from the workspace, untouched = dict name -> the output still holds only sentinel bytes, ws)."""
    import torch
    from pytorch_sparse_amd import _native as nat
    L = nat.lib()
    dev = row.device
    E = row.numel()
    i64, sz = ctypes.c_int64, ctypes.c_size_t
    coalesce = entry != 'values'
    nws = (L.tsamd_sort_coalesce_workspace_bytes if coalesce else L.tsamd_sort_coo_workspace_bytes)(i64(E))
    if ws is None:
        ws = Guarded(nws, dev, WS_SENT)
    assert ws.nbytes == nws
    vb = 0 if value is None else value.element_size()
    g = {}
    if coalesce:
        for name in ('row_tmp', 'col_tmp', 'row_u', 'col_u'):
            g[name] = Guarded(8 * E, dev)
        g['seg_ptr'] = Guarded(8 * (E + 1), dev)
        g['counts'] = Guarded(8 * (4 if entry == 'reduce' else 3), dev)
    else:
        for name in ('row_out', 'col_out', 'perm_out'):
            g[name] = Guarded(8 * E, dev)
        g['counts'] = Guarded(8 * 4, dev)
        if mode == 2:
            g['counts'].body(torch.int64).copy_(counts_in)
    if value is not None:
        g['value_out'] = Guarded(vb * E, dev)
        if entry == 'reduce':
            g['value_u'] = Guarded(vb * E, dev)
    p = {k: v.ptr for k, v in g.items()}
    none = ctypes.c_void_p(0)
    with torch.cuda.device(dev):
        stream = nat.stream_ptr(dev)
        if entry == 'values':
            st = L.tsamd_sort_coo_values(mode, nat._ptr(row), nat._ptr(col), i64(E), i64(M), i64(N), p['row_out'],
                                         p['col_out'], p['perm_out'], none if mode == 0 else p['counts'], nat._ptr(value),
                                         p.get('value_out', none), i64(vb), ws.ptr, sz(ws.nbytes), stream)
        elif entry == 'coalesce':
            st = L.tsamd_sort_coalesce(nat._ptr(row), nat._ptr(col), i64(E), i64(M), i64(N), p['row_tmp'], p['col_tmp'],
                                       p['row_u'], p['col_u'], p['seg_ptr'], p['counts'], nat._ptr(value),
                                       p.get('value_out', none), i64(vb), ws.ptr, sz(ws.nbytes), stream)
        else:
            assert entry == 'reduce' and (value is None or value.dtype in (torch.float32, torch.int32))
            dt = nat.DTYPES[torch.int32 if value is not None and value.dtype == torch.int32 else torch.float32]
            st = L.tsamd_sort_coalesce_reduce(nat._ptr(row), nat._ptr(col), i64(E), i64(M), i64(N), p['row_tmp'],
                                              p['col_tmp'], p['row_u'], p['col_u'], p['seg_ptr'], p['counts'], dt, reduce,
                                              nat._ptr(value), p.get('value_out', none), p.get('value_u', none), ws.ptr,
                                              sz(ws.nbytes), stream)
        torch.cuda.synchronize(dev)
    guards_ok = ws.intact() and all(v.intact() for v in g.values())
    off, w_desc, w_fast, w_err = header(E, 1 if coalesce else 0)
    words = ws.body()[off:off + 64 * 8].view(torch.int64).tolist()
    hdr = {'descents': words[w_desc], 'fast': words[w_fast], 'error': words[w_err]}
    out = {}
    for k, v in g.items():
        if k in ('value_out', 'value_u'):
            out[k] = v.body(value.dtype)
        else:
            out[k] = v.body(torch.int64)
    untouched = {k: v.untouched() for k, v in g.items()}
    return Result(int(st), out, guards_ok, hdr, untouched, ws)
