"""Reference of the CSR SpMM forward (csrc/spmm_kernels.h): an fp64 oracle with the contract of reducer.h as restated
at the top of that header, a linear oracle for graphs over few columns, the two comparators of the route tests with
derived bounds, the merge-path partition in numpy, a census of what a call's partition does to its rows (and of what
the short-row kernel's batching decides), a restatement of the product piece by piece whose switches plant defects,
and the graphs ("builders") that reach each route.  numpy and torch on the CPU only; no compiled code.

Operands are fp64 numpy arrays holding values the element type represents exactly (torch tensors of the element type
are made from them where a result is compared bit for bit); element types are torch dtypes."""
import numpy as np
import torch

FLOATS = (torch.float32, torch.float64, torch.float16, torch.bfloat16)
REDUCES = ('sum', 'mean', 'min', 'max')
# unit roundoff 2^-p of the element type (p significant bits) and of the accumulator (fp32 for fp32 / f16 / bf16)
U_OUT = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
U_ACC = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -24}
# Traits<T>::max_init (min starts there; lowest_init is its negative): the largest finite element
INIT = {torch.float32: 3.4028234663852886e+38, torch.float64: 1.7976931348623157e+308, torch.float16: 65504.0,
        torch.bfloat16: 3.3895313892515355e+38}
# the project's comparator (tests/util.py: the BASELINE bar); the derived bound may only be the tighter of the two
SUM_TOL = {torch.float32: 1e-5, torch.float64: 1e-13, torch.float16: 2e-3, torch.bfloat16: 1.6e-2}
SUM_ATOL = {torch.float32: 1e-37, torch.float64: 1e-300, torch.float16: 6e-8, torch.bfloat16: 1e-37}
# half the spacing of the subnormals of a narrower output type: what one rounding costs below the normal range
TINY = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
SHORT_FACTOR = 8  # kShortFactor: rows of more than 8 * lpr entries leave a short-row batch
WAVE = 64
DEFECTS = ('head_drops_last_entry', 'middle_piece_skipped', 'fold_stops_at_64', 'fold_stops_at_full_batches',
           'tie_to_larger_id', 'tail_widened_with_wrong_partition', 'mean_by_piece_length', 'last_packet_skipped',
           'batch1_reads_batch0', 'limit_row_loses_last_entry', 'empty_row_keeps_previous')


# ---- element types ----------------------------------------------------------------------------------------------
def store(a, dtype):
    """fp64 numbers -> torch tensor of `dtype`, rounded once (f16 beyond 65504 -> +-inf)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)


def rounded(a, dtype):
    """fp64 numbers rounded once to `dtype`, as fp64 again."""
    if dtype == torch.float64:
        return np.asarray(a, np.float64)
    return store(a, dtype).double().numpy()


def _products(value, x, col, s, e, dtype, minmax):
    """value * x rows of entries [s, e) in fp64 (exact: both factors have <= 24 bits, or are fp64 themselves); min / max
    see them rounded to the element type (reducer.h:63-67: the product is a scalar_t before the reducer sees it)."""
    p = x[col[s:e]]
    if value is not None:
        p = value[s:e, None] * p
        if minmax and dtype is not None:
            p = rounded(p, dtype)
    return p


def _batched(x):
    x = np.asarray(x, np.float64)
    return (x[None], False) if x.ndim == 2 else (x, True)


# ---- oracle -----------------------------------------------------------------------------------------------------
def oracle_loops(rowptr, col, value, x, reduce, dtype=None):
    """The contract, entry by entry: -> (exact [B,] M, K fp64, sum of |terms| (None for min / max), ids or None).
    sum / mean: empty rows give 0, the mean divides by max(row length, 1).  min / max: start at -+INIT[dtype], strict
    compares (the first occurrence wins a tie, NaN never wins), a row without a winner reports E and the init value,
    an empty row 0 and E."""
    xb, batched = _batched(x)
    M, E, K = len(rowptr) - 1, len(col), xb.shape[2]
    minmax = reduce in ('min', 'max')
    out = np.zeros((xb.shape[0], M, K), np.longdouble if dtype == torch.float64 and not minmax else np.float64)
    l1 = None if minmax else np.zeros_like(out)
    arg = np.full((xb.shape[0], M, K), E, np.int64) if minmax else None
    init = INIT[dtype if dtype is not None else torch.float64]
    for b in range(xb.shape[0]):
        for r in range(M):
            s, e = int(rowptr[r]), int(rowptr[r + 1])
            if minmax:
                if s == e:
                    continue
                val = np.full(K, init if reduce == 'min' else -init)
                for i in range(s, e):
                    p = _products(value, xb[b], col, i, i + 1, dtype, True)[0]
                    better = (p < val) if reduce == 'min' else (p > val)
                    val = np.where(better, p, val)
                    arg[b, r] = np.where(better, i, arg[b, r])
                out[b, r] = val
            else:
                for i in range(s, e):
                    p = _products(value, xb[b], col, i, i + 1, dtype, False)[0]
                    out[b, r] += p
                    l1[b, r] += np.abs(p)
                if reduce == 'mean':
                    out[b, r] /= max(e - s, 1)
                    l1[b, r] /= max(e - s, 1)
    if not batched:
        return out[0], (None if l1 is None else l1[0]), (None if arg is None else arg[0])
    return out, l1, arg


def oracle(rowptr, col, value, x, reduce, dtype=None, chunk=1 << 23):
    """oracle_loops vectorised (np.*.reduceat over blocks of rows of <= `chunk` products); fp64 sums accumulate in
    long double, so that the oracle's own error stays 2^-11 of the fp64 bound."""
    xb, batched = _batched(x)
    rowptr = np.asarray(rowptr, np.int64)
    M, E, K = len(rowptr) - 1, len(col), xb.shape[2]
    minmax = reduce in ('min', 'max')
    wide = np.longdouble if dtype == torch.float64 and not minmax else np.float64
    out = np.zeros((xb.shape[0], M, K), wide)
    l1 = None if minmax else np.zeros_like(out)
    arg = np.full((xb.shape[0], M, K), E, np.int64) if minmax else None
    init = INIT[dtype if dtype is not None else torch.float64]
    deg = rowptr[1:] - rowptr[:-1]
    r = 0
    while r < M:
        r2 = int(np.searchsorted(rowptr, rowptr[r] + max(chunk // K, 1), side='right'))
        r2 = min(max(r2 - 1, r + 1), M)
        s, e = int(rowptr[r]), int(rowptr[r2])
        rows = np.nonzero(deg[r:r2] > 0)[0] + r
        if e > s:
            starts = rowptr[rows] - s
            for b in range(xb.shape[0]):
                p = _products(value, xb[b], col, s, e, dtype, minmax)
                if not minmax:
                    out[b, rows] = np.add.reduceat(p.astype(wide), starts, axis=0)
                    l1[b, rows] = np.add.reduceat(np.abs(p).astype(wide), starts, axis=0)
                    continue
                sgn = -1.0 if reduce == 'min' else 1.0
                q = sgn * p
                with np.errstate(invalid='ignore'):
                    valid = q > -init  # strict against the init value; NaN fails
                cand = np.where(valid, q, -np.inf)
                m = np.maximum.reduceat(cand, starts, axis=0)  # [rows, K]
                seg = np.repeat(np.arange(len(rows)), deg[rows])
                ids = np.arange(s, e, dtype=np.int64)[:, None]
                first = np.minimum.reduceat(np.where(valid & (cand == m[seg]), ids, E), starts, axis=0)
                has = first < E
                at = np.where(has, first - s, 0)
                won = np.take_along_axis(p, at, axis=0)  # the winner's own bits (+0.0 and -0.0 compare equal)
                out[b, rows] = np.where(has, won, -sgn * init)
                arg[b, rows] = first
        r = r2
    if reduce == 'mean':
        d = np.maximum(deg, 1)[None, :, None]
        out, l1 = out / d, l1 / d
    if not batched:
        return out[0], (None if l1 is None else l1[0]), (None if arg is None else arg[0])
    return out, l1, arg


def oracle_int(rowptr, col, value, x, reduce, dtype):
    """Integer types wrap and their mean truncates: the C oracle (oracle/c_oracle.py) pins that; torch tensors in,
    (out, ids or None) as torch tensors out."""
    from tests.util import oracle_spmm
    return oracle_spmm(rowptr, col, value, x, reduce)


def linear_oracle(rowptr, col, value, x, reduce, N):
    """sum / mean over few columns: S[r, c] = sum of the values of the entries (r, c) by a weighted bincount in fp64,
    then S @ X; the same with absolute values for the sum of |terms|.  Exact while the operands are small integers."""
    rowptr = np.asarray(rowptr, np.int64)
    M, x = len(rowptr) - 1, np.asarray(x, np.float64)
    deg = rowptr[1:] - rowptr[:-1]
    key = np.repeat(np.arange(M, dtype=np.int64), deg) * N + col
    w = np.ones(len(col)) if value is None else np.asarray(value, np.float64)
    S = np.bincount(key, weights=w, minlength=M * N).reshape(M, N)
    Sa = np.bincount(key, weights=np.abs(w), minlength=M * N).reshape(M, N)
    out, l1 = S @ x, Sa @ np.abs(x)
    if reduce == 'mean':
        d = np.maximum(deg, 1)[:, None]
        out, l1 = out / d, l1 / d
    return out, l1


def linear_minmax(rowptr, col, x, reduce, N, dtype, rows_per_step=64):
    """min / max without values over few columns: the winner of row r is the best x[c] over the columns the row names;
    its id is the first entry of the row whose column attains it."""
    rowptr = np.asarray(rowptr, np.int64)
    M, E, x = len(rowptr) - 1, len(col), np.asarray(x, np.float64)
    K = x.shape[1]
    deg = rowptr[1:] - rowptr[:-1]
    key = np.repeat(np.arange(M, dtype=np.int64), deg) * N + col
    first = np.full(M * N, E, np.int64)
    first[key[::-1]] = np.arange(E, dtype=np.int64)[::-1]  # (a repeated index keeps the last value assigned: the first id)
    first = first.reshape(M, N)
    sgn = -1.0 if reduce == 'min' else 1.0
    init = INIT[dtype]
    q = sgn * x
    with np.errstate(invalid='ignore'):
        ok_x = q > -init
    out, arg = np.zeros((M, K)), np.full((M, K), E, np.int64)
    for r in range(0, M, rows_per_step):
        f = first[r:r + rows_per_step]
        pres = (f < E)[:, :, None] & ok_x[None]
        cand = np.where(pres, q[None], -np.inf)
        m = cand.max(axis=1)
        a = np.where(pres & (cand == m[:, None, :]), f[:, :, None], E).min(axis=1)
        has = a < E
        won = x[col[np.where(has, a, 0)], np.arange(K)[None, :]]
        out[r:r + rows_per_step] = np.where(has, won, -sgn * init)
        arg[r:r + rows_per_step] = a
    empty = deg == 0
    out[empty] = 0.0
    return out, arg


# ---- comparators ------------------------------------------------------------------------------------------------
def bits_of(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def exact_operands_ok(rowptr, dtype):
    """Exact mode: |value| <= 4 and |x| <= 8 (f16: 1 and 2) are integers, so every partial sum of a row shorter than
    2^24 / 32 is an integer below 2^24: exact in a 4-byte accumulator in any order; f16 results stay finite."""
    deg = int(np.max(np.diff(rowptr))) if len(rowptr) > 1 else 0
    return deg < (1 << 24) // 32 and (dtype != torch.float16 or deg * 2 <= 65504)


def exact_mismatches(got, exact, dtype):
    """Number of output elements whose bits differ from the exact result rounded once to `dtype`.  No element is
    excluded."""
    want = store(np.asarray(exact, np.float64), dtype)
    assert bool(torch.isfinite(want).all()) or dtype != torch.float16, 'builder let an f16 result overflow'
    return int((bits_of(got) != bits_of(want.reshape(got.shape))).sum())


def real_bound(exact, l1, rowptr, dtype, reduce):
    """|got - exact| <= (deg + 2) u_acc sum|terms| + u_out |exact|: deg products and additions of relative error u_acc
    each (gamma_deg to first order; the + 2 covers the higher orders and the fold of a cut row's pieces), + 1 for the
    mean's division, and the one rounding to a narrower output type (relative u_out, or half a subnormal step where
    the result is that small: f16 results below 6e-5 are not relatively accurate).  Never looser than the project's
    comparator."""
    deg = np.diff(np.asarray(rowptr, np.int64)).astype(np.float64)
    deg = deg.reshape((1, ) * (np.ndim(exact) - 2) + (-1, 1)) + (1.0 if reduce == 'mean' else 0.0)
    l1 = np.asarray(l1, np.float64)
    u_out = 0.0 if U_OUT[dtype] == U_ACC[dtype] else U_OUT[dtype]
    derived = (deg + 2.0) * U_ACC[dtype] * l1 + np.maximum(u_out * np.abs(np.asarray(exact, np.float64)), TINY[dtype])
    return np.minimum(derived, SUM_TOL[dtype] * l1 + SUM_ATOL[dtype])


def real_violations(got, exact, l1, rowptr, dtype, reduce):
    """-> (number of elements outside real_bound, the largest error / bound).  No element is excluded."""
    g = got.detach().cpu()
    g = g.numpy().astype(np.longdouble) if dtype == torch.float64 else g.double().numpy()
    err = np.abs(g - np.asarray(exact).reshape(g.shape)).astype(np.float64)
    bound = real_bound(np.asarray(exact, np.float64).reshape(g.shape), np.asarray(l1, np.float64).reshape(g.shape),
                       rowptr, dtype, reduce)
    bad = ~(err <= bound)  # (a NaN error counts)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return int(bad.sum()), float(np.nanmax(ratio)) if ratio.size else 0.0


def minmax_mismatches(got, got_arg, exact, arg, dtype):
    """min / max: values bit for bit and ids, always."""
    want = store(exact, dtype)
    return int((bits_of(got) != bits_of(want.reshape(got.shape))).sum()) + \
        int((got_arg.detach().cpu().to(torch.int64) != torch.from_numpy(np.asarray(arg)).reshape(got_arg.shape)).sum())


# ---- operands ---------------------------------------------------------------------------------------------------
def exact_operands(N, K, E, dtype, seed, B=None):
    """Small non-zero integers: dropping, doubling or misplacing one term changes the exact sum."""
    rng = np.random.default_rng(seed)
    vmax, xmax = (1, 2) if dtype == torch.float16 else (4, 8)
    v = rng.integers(1, vmax + 1, E) * rng.choice([-1.0, 1.0], E)
    shape = (N, K) if B is None else (B, N, K)
    x = rng.integers(1, xmax + 1, shape) * rng.choice([-1.0, 1.0], shape)
    return v.astype(np.float64), x.astype(np.float64)


def real_operands(N, K, E, dtype, seed, B=None):
    """Real values the element type represents: standard normal features, values in +-[0.2, 1.2)."""
    g = torch.Generator().manual_seed(seed)
    shape = (N, K) if B is None else (B, N, K)
    x = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype if dtype != torch.float64 else torch.float32)
    v = (torch.rand(E, generator=g, dtype=torch.float64) + 0.2) * (torch.randint(0, 2, (E, ), generator=g) * 2 - 1)
    v = v.to(dtype if dtype != torch.float64 else torch.float32)
    return v.double().numpy(), x.double().numpy()


# ---- merge-path partition ---------------------------------------------------------------------------------------
def partition(rowptr, items, snap=0):
    """spmm_partition_kernel: P + 1 diagonal searches over (row ends, entries), then the snap to row starts
    -> int64 [P + 1, 2] of (row, entry)."""
    rowptr = np.asarray(rowptr, np.int64)
    M, E = len(rowptr) - 1, int(rowptr[-1])
    total = max(M + E, 1)
    P = -(-total // items)
    d = np.minimum(np.arange(P + 1, dtype=np.int64) * items, M + E)
    # the search's predicate rowptr[mid + 1] <= d - mid - 1 is monotone in mid: count where it holds
    keys = rowptr[1:] + np.arange(1, M + 1, dtype=np.int64)
    lo = np.clip(np.searchsorted(keys, d, side='right'), np.maximum(d - E, 0), np.minimum(d, M))
    e = d - lo
    if snap > 0:
        rs = rowptr[np.minimum(lo, M)]
        move = (lo < M) & (e > rs) & (e - rs <= snap)
        e = np.where(move, rs, e)
    return np.stack([lo, e], axis=1)


def row_records(rowptr, table):
    """What the merge kernel leaves per partition: tail_row (the unfinished last row whose piece here has entries, or
    -1) and head_row (the cut first row when it ends here, or -1)."""
    rowptr, table = np.asarray(rowptr, np.int64), np.asarray(table, np.int64)
    M = len(rowptr) - 1
    r0, e0, r1, e1 = table[:-1, 0], table[:-1, 1], table[1:, 0], table[1:, 1]
    incoming = (r0 < M) & (e0 > rowptr[np.minimum(r0, M)])
    tail = (r1 < M) & (e1 > np.maximum(e0, rowptr[np.minimum(r1, M)]))
    return np.where(tail, r1, -1), np.where(incoming & (r1 > r0), r0, -1)


def census(rowptr, table, items, snap=0, tail_row=None, head_row=None):
    """What a partition does to the rows.  `table`: the device's, or partition(...); tail_row / head_row: the device's,
    held to row_records.  Decides nothing about expected values."""
    rowptr, table = np.asarray(rowptr, np.int64), np.asarray(table, np.int64)
    M, P = len(rowptr) - 1, len(table) - 1
    t_want, h_want = row_records(rowptr, table)
    if tail_row is not None:
        assert np.array_equal(np.asarray(tail_row), t_want), 'tail_row differs from the partition table'
        assert np.array_equal(np.asarray(head_row), h_want), 'head_row differs from the partition table'
    r0, e0, r1, e1 = table[:-1, 0], table[:-1, 1], table[1:, 0], table[1:, 1]
    incoming = (r0 < M) & (e0 > rowptr[np.minimum(r0, M)])
    runs = {}
    for q in np.nonzero(h_want >= 0)[0]:
        run, R = 0, h_want[q]
        while q - 1 - run >= 0 and t_want[q - 1 - run] == R:
            run += 1
        runs[int(R)] = run
    hist = {}
    for run in runs.values():
        hist[run] = hist.get(run, 0) + 1
    plain = partition(rowptr, items, 0)
    return {
        'P': P, 'cut_rows': len(runs), 'run_hist': hist, 'runs': runs,
        'inside_one_row': int(((r0 == r1) & (e1 > e0)).sum()),
        'incoming_row_ends': int((incoming & (r1 > r0)).sum()),
        'boundary_on_row_start': int(((r1 < M) & (e1 == rowptr[np.minimum(r1, M)]))[:-1].sum()),
        # every entry of the row consumed, its row end not: the head piece in the next partition is empty
        'empty_head': int((incoming & (e0 == rowptr[np.minimum(r0 + 1, M)])).sum()),
        'empty_partitions': int((e0 == e1).sum()),
        'cut_last_row': int(M - 1 in runs),
        'snapped': int((plain[:, 1] != table[:, 1]).sum()) if len(plain) == len(table) else -1,
    }


def short_census(rowptr, table, lgG):
    """The short-row kernel's batching decision (short_rows / short_row_batches of spmm_merge_kernel) restated per
    partition: which rows go side by side, and why a batch is refused or ends."""
    rowptr, table = np.asarray(rowptr, np.int64), np.asarray(table, np.int64)
    M, G, lpr = len(rowptr) - 1, 1 << lgG, 64 >> lgG
    limit = SHORT_FACTOR * lpr
    c = {'batches': 0, 'rows_in_batches': 0, 'ended_by_long_0': 0, 'ended_by_long_1': 0, 'ended_by_long_2plus': 0,
         'navail_lt2': 0, 'reloads': 0, 'longest_batch': 0, 'incoming_then_batch': 0, 'unfinished_short_last': 0,
         'limit_row_member_0': 0, 'limit_row_member_1': 0, 'limit_row_member_2plus': 0,
         'over_limit_member_0': 0, 'over_limit_member_1': 0, 'over_limit_member_2plus': 0, 'batch_sizes': {}}
    cls = lambda g: '0' if g == 0 else ('1' if g == 1 else '2plus')  # noqa: E731
    for p in range(len(table) - 1):
        (r0, e0), (r1, e1) = table[p], table[p + 1]
        incoming = r0 < M and e0 > rowptr[r0]
        st = {'r': int(r0), 'base': int(r0)}

        def short_rows():
            r = st['r']
            if lgG < 3 or r >= r1:
                return False
            j = r - st['base']
            if j >= WAVE:
                st['base'], j = r, 0
                c['reloads'] += 1
            navail = min(r1 - r, G, WAVE - j)
            if navail < 2:
                c['navail_lt2'] += 1
                return False
            lens = rowptr[r + 1:r + navail + 1] - rowptr[r:r + navail]
            long_at = np.nonzero(lens > limit)[0]
            n = int(long_at[0]) if len(long_at) else int(navail)
            if len(long_at):
                c['ended_by_long_' + cls(n)] += 1
                if lens[n] == limit + 1:
                    c['over_limit_member_' + cls(n)] += 1
            if n < 2:
                return False
            for g in np.nonzero(lens[:n] == limit)[0]:
                c['limit_row_member_' + cls(int(g))] += 1
            c['batches'] += 1
            c['rows_in_batches'] += n
            c['batch_sizes'][n] = c['batch_sizes'].get(n, 0) + 1
            c['longest_batch'] = max(c['longest_batch'], n)
            st['r'] = r + n
            return True

        def batches():
            if not short_rows():
                return False
            while short_rows():
                pass
            return True
        if not incoming:
            batches()
        while st['r'] < r1:  # the cooperative path finishes one row, then looks for short ones again
            first = st['r'] == r0 and incoming
            if st['r'] - st['base'] == WAVE:
                st['base'] = st['r']
            st['r'] += 1
            if batches() and first:
                c['incoming_then_batch'] += 1
        if r1 < M and e1 > max(e0, rowptr[r1]) and rowptr[r1 + 1] - rowptr[r1] <= limit:
            c['unfinished_short_last'] += 1
    return c


# ---- the product piece by piece ---------------------------------------------------------------------------------
def piecewise(rowptr, col, value, x, reduce, dtype, route, table, defect=None):
    """The three kernels restated: every partition reduces its rows -- and row pieces -- in the accumulator type
    (4 bytes for fp32 / f16 / bf16), leaves head / tail records for the rows it shares, and the fix-up folds a cut
    row's records from the partition in which it ends backwards (fp64 fold for fp32 sums; min / max ties to the
    smaller id).  -> (out as a torch tensor of `dtype`, ids or None).  `defect`: one of DEFECTS, planted."""
    assert defect is None or defect in DEFECTS
    rowptr, table = np.asarray(rowptr, np.int64), np.asarray(table, np.int64)
    xb, batched = _batched(x)
    B, M, E, K, P = xb.shape[0], len(rowptr) - 1, len(col), xb.shape[2], len(table) - 1
    minmax, mean = reduce in ('min', 'max'), reduce == 'mean'
    acc = np.float64 if dtype == torch.float64 else np.float32
    sgn = -1.0 if reduce == 'min' else 1.0
    init = acc(INIT[dtype])
    vec, lpr = route['vec'], route['lpr']
    kdone = K  # features [kdone, K) of the last packet are never accumulated (defect)
    if defect == 'last_packet_skipped' and K % (WAVE * vec) != 0:
        kdone = (route['slots'] - 1) * vec
    out = np.zeros((B, M, K), acc)
    arg = np.full((B, M, K), E, np.int64) if minmax else None
    NOARG = np.iinfo(np.int64).max

    def piece(b, s, e, first_edge):
        """entries [s, e) of one row -> (value, winner offset from `first_edge` or NOARG)"""
        xs = xb[0 if (defect == 'batch1_reads_batch0' and b == 1) else b]
        if not minmax:
            v = np.zeros(K, acc)
            if e > s:
                p = _products(value, xs, col, s, e, dtype, False).astype(acc)
                v[:kdone] = p[:, :kdone].sum(axis=0, dtype=acc)
            return v, None
        v, a = np.full(K, -sgn * init, acc), np.full(K, NOARG, np.int64)
        if e > s:
            q = sgn * _products(value, xs, col, s, e, dtype, True).astype(acc)
            with np.errstate(invalid='ignore'):
                valid = q > -init
            cand = np.where(valid, q, -np.inf)
            m = cand.max(axis=0)
            at = np.where(valid & (cand == m), np.arange(s, e)[:, None], NOARG).min(axis=0)
            has = at < NOARG
            won = np.take_along_axis(sgn * q, np.where(has, at - s, 0)[None], axis=0)[0]
            v, a = np.where(has, won, v).astype(acc), np.where(has, at - first_edge, NOARG)
            v[kdone:], a[kdone:] = -sgn * init, NOARG
        return v, a

    def finish(b, r, v, a, length, deg):
        """write_row: `length` decides empty, `deg` divides the mean"""
        if minmax:
            if length > 0:
                out[b, r] = v
                arg[b, r] = np.where(a == NOARG, E, a)
            else:
                out[b, r], arg[b, r] = 0, E
        else:
            out[b, r] = (v / acc(max(deg, 1))).astype(acc) if mean else v
        if defect == 'empty_row_keeps_previous' and length == 0 and r > 0:
            out[b, r] = out[b, r - 1]
            if minmax:
                arg[b, r] = arg[b, r - 1]

    tail_row, head_row = row_records(rowptr, table)
    for b in range(B):
        head, tail = [None] * P, [None] * P
        for p in range(P):
            (r0, e0), (r1, e1) = (int(t) for t in table[p]), (int(t) for t in table[p + 1])
            incoming = r0 < M and e0 > rowptr[r0]
            for r in range(r0, r1):
                s, e = max(e0, int(rowptr[r])), int(rowptr[r + 1])
                if incoming and r == r0:
                    if defect == 'head_drops_last_entry' and e > s:
                        e -= 1
                    head[p] = piece(b, s, e, e0) + (e - s, )
                    continue
                if defect == 'limit_row_loses_last_entry' and e - s == SHORT_FACTOR * lpr:
                    v, a = piece(b, s, e - 1, 0)
                else:
                    v, a = piece(b, s, e, 0)
                finish(b, r, v, a, int(rowptr[r + 1] - rowptr[r]), e - s)
            if tail_row[p] >= 0:
                tail[p] = piece(b, max(e0, int(rowptr[r1])), e1, e0)
        for q in range(1, P):
            R = int(head_row[q])
            if R < 0:
                continue
            run = 0
            while q - 1 - run >= 0 and tail_row[q - 1 - run] == R:
                run += 1
            if defect == 'fold_stops_at_64':
                run = min(run, 64)
            if defect == 'fold_stops_at_full_batches' and run > 1:
                run = 1 + (run - 1) // 8 * 8
            hv, ha, hlen = head[q]
            widen = lambda a, p: np.where(a == NOARG, NOARG, a + table[p, 1])  # noqa: E731
            if minmax:
                val, wa = hv.copy(), widen(ha, q)
            else:
                val = hv.astype(np.float64) if acc == np.float32 else hv.copy()
            for i in range(run):
                p = q - 1 - i
                if defect == 'middle_piece_skipped' and run >= 2 and i == run // 2:
                    continue
                tv, ta = tail[p]
                if not minmax:
                    val = val + tv
                    continue
                ta = widen(ta, p + 1 if defect == 'tail_widened_with_wrong_partition' else p)
                tq, vq = sgn * tv, sgn * val
                tie = (ta > wa) if defect == 'tie_to_larger_id' else (ta < wa)
                take = (tq > vq) | ((tq == vq) & tie)
                val, wa = np.where(take, tv, val), np.where(take, ta, wa)
            deg = int(rowptr[R + 1] - rowptr[R])
            finish(b, R, val.astype(acc), wa if minmax else None, deg, hlen if defect == 'mean_by_piece_length' else deg)
    o = torch.from_numpy(out if batched else out[0]).to(dtype)
    return o, (None if arg is None else (arg if batched else arg[0]))


# ---- builders ---------------------------------------------------------------------------------------------------
class Rows:
    """Rows laid along the merge path: every row takes len + 1 items (its entries, then its row end)."""

    def __init__(self, items):
        self.items, self.lens = items, []
        self.diag = 0

    def add(self, *lens):
        for n in lens:
            self.lens.append(int(n))
            self.diag += int(n) + 1
        return len(self.lens) - 1

    def align(self, offset=0):
        """empty rows until the next row starts `offset` items behind a partition boundary"""
        pad = (offset - self.diag) % self.items
        self.add(*([0] * pad))

    def rowptr(self):
        return np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)


def columns(E, N, seed):
    return np.random.default_rng(seed).integers(0, N, E).astype(np.int64)


CHAIN_PIECES = (2, 3, 8, 9, 10, 17, 64, 65, 66, 129, 200)


def build_chains(items, seed=0):
    """Cut rows of every chain length the fix-up kernel branches on (run = pieces - 1 tail records: 1, 2..8, 9 and
    more in batches of 8 plus a remainder, exactly 64, more than 64, 128 and more), rows cut one entry behind their
    start and one entry before their end, a boundary exactly on a row's last entry (empty head), a hub followed by 300
    empty rows, short filler rows, and a cut last row.  -> (rowptr, census keys it must reach)."""
    rng = np.random.default_rng(seed)
    g = Rows(items)
    for pieces in CHAIN_PIECES:
        g.align()
        g.add((pieces - 1) * items + int(rng.integers(1, items - 1)))  # starts on a boundary: `pieces` pieces
        g.add(*rng.integers(0, 9, 5))
    g.align(items - 1)
    g.add(40)                       # one entry, then the boundary
    g.align(items - 38)
    g.add(39)                       # the boundary, then the last entry
    g.align()
    g.add(items)                    # every entry in one partition, the row end in the next: an empty head piece
    g.align(5)
    g.add(3 * items)                # a hub ...
    g.add(*([0] * 300))             # ... and 300 empty rows behind it
    g.add(*rng.integers(0, 30, 40))
    g.align(10)
    g.add(2 * items)                # the matrix ends inside a cut row
    keys = {'run_hist': [p - 1 for p in CHAIN_PIECES], 'empty_head': 1, 'cut_last_row': 1, 'inside_one_row': 1,
            'boundary_on_row_start': 1, 'incoming_row_ends': 1}
    return g.rowptr(), keys


def build_one_row(items):
    return np.array([0, 3 * items + 5], np.int64), {'run_hist': [3], 'cut_last_row': 1}


def build_partitions(items, P, seed=0):
    """M + E <= items (one partition: no fix-up launch) or in (items, 2 items]."""
    rng = np.random.default_rng(seed)
    M = 9
    lens = rng.multinomial(P * items - M - 3, np.ones(M) / M)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), {'P': P}


def build_skewed(M, seed=0, mean_len=16, hub=600):
    """2^10-row style census graph: power-law row lengths with empty rows and a few hubs, so rows are cut and the
    fix-up runs whatever the packet width."""
    rng = np.random.default_rng(seed)
    lens = np.minimum((rng.pareto(1.1, M) * mean_len * 0.3).astype(np.int64), hub)
    lens[rng.integers(0, M, M // 16)] = 0
    lens[rng.integers(0, M, 3)] = hub
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), {'cut_rows': 1}


def build_ties(items, snap, seed=0):
    """Rows for the winner cases: 0 a 70-piece row (all entries equal, or a unique winner per feature in its first /
    a middle / its last piece), 1 a cut row of NaN, 2 a cut row of +-0.0, then -- with `snap` -- a row of exactly `snap`
    entries and one of snap + 1 that a boundary would cut one entry before their end.  -> (rowptr, keys, named rows)."""
    g = Rows(items)
    named = {}
    g.align()
    named['long'] = g.add(69 * items + 7)
    g.add(3, 0, 5)
    first = max(snap, 20) + 10  # entries in front of the first boundary: more than `snap`, so that it stays
    g.align(items - first)
    named['nan'] = g.add(items + 20)
    g.add(2, 2)
    g.align(items - first)
    named['zeros'] = g.add(2 * items)
    g.add(1, 4)
    if snap > 0:
        g.align(items - snap + 1)
        named['snap'] = g.add(snap)       # the boundary falls snap - 1 entries in: it moves back, the row is whole
        g.add(3)
        g.align(items - snap - 1)
        named['snap1'] = g.add(snap + 1)  # snap + 1 entries in (all of them; the row end is behind it): it stays, cut
        g.add(2, 6)
    return g.rowptr(), {'run_hist': [69]}, named


def build_short(items, lgG, seed=0):
    """Short-row batches: rows of exactly 8 lpr and of 8 lpr + 1 entries as the first, second and a middle member of
    a batch; runs of 1, 2, G and G + 1 short rows between long ones; 200 consecutive empty rows; short rows behind a
    cut row's end; random short filler so partitions end inside short rows.  -> (rowptr, short-census keys)."""
    rng = np.random.default_rng(seed)
    G, lpr = 1 << lgG, 64 >> lgG
    limit = SHORT_FACTOR * lpr
    g = Rows(items)
    long_row = limit + 5
    for member in (0, 1, min(3, G - 1)):
        for length in (limit, limit + 1):
            g.align()  # the batch starts with the partition, so `length` is its member number `member`
            g.add(*rng.integers(1, 4, member))
            g.add(length)
            g.add(*rng.integers(1, 4, 3))
    for run in (1, 2, G, G + 1):
        g.align()
        g.add(long_row)
        g.add(*rng.integers(0, 3, run))
        g.add(long_row)
    g.align()
    g.add(long_row, 2, items)  # one short row between a long one and the partition's cut last row: navail < 2
    g.add(long_row)
    g.add(*([0] * 200))
    g.align(items - 20)
    g.add(3 * items)  # a cut row; the partition in which it ends goes on with short rows
    g.add(*rng.integers(1, 5, 40))
    for _ in range(12):
        g.add(*rng.integers(0, min(limit, 12) + 1, 30))
        g.add(limit)
    keys = ['batches', 'ended_by_long_0', 'ended_by_long_1', 'ended_by_long_2plus', 'navail_lt2', 'reloads',
            'incoming_then_batch', 'unfinished_short_last', 'limit_row_member_0', 'limit_row_member_1',
            'limit_row_member_2plus', 'over_limit_member_0', 'over_limit_member_1', 'over_limit_member_2plus']
    return g.rowptr(), keys


TARGET_WAVES = 32768
# (element type, K, M + E, items) of the partition-length cases: a length in 129..255 that is no multiple of 64 (two),
# 256, one in 257..511 and 512 itself (513..1023-byte rows), 1024 for rows of 1 KB, 1024 for rows of <= 128 bytes
LENGTH_CASES = [(torch.float32, 64, 200 * TARGET_WAVES - 77, 200), (torch.bfloat16, 64, 150 * TARGET_WAVES - 5, 150),
                (torch.float32, 64, 256 * TARGET_WAVES + 9, 256), (torch.float32, 132, 300 * TARGET_WAVES - 1, 300),
                (torch.bfloat16, 260, 512 * TARGET_WAVES + 3, 512), (torch.float32, 256, 1024 * TARGET_WAVES + 1, 1024),
                (torch.float32, 16, 1024 * TARGET_WAVES + 1, 1024)]


def build_total(M, total, seed=0):
    """M rows of skewed lengths with M + E == total exactly (the partition-length cases: `items` follows M + E)."""
    rng = np.random.default_rng(seed)
    w = rng.pareto(1.5, M) + 0.05
    w = np.minimum(w, 40 * w.mean())  # (the longest row stays below 2^19 entries at 33 M: exact mode)
    w[rng.integers(0, M, M // 8)] = 0
    E = total - M
    lens = np.floor(w / w.sum() * E).astype(np.int64)
    lens[int(np.argmax(lens))] += E - int(lens.sum())
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
