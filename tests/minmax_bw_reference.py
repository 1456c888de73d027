"""Reference of the min / max backward of CSR SpMM (csrc/spmm_bw.hip, the record-writing forward and the masked sum of
csrc/spmm_kernels.h).  No kernel takes part: the winners come from tests/spmm_forward_reference.py (exact `out` and
`arg`, first occurrence on a tie), the gradients follow the three lines of the reference's backward in fp64 (long double
sums), the winner records restate the layout of csrc/spmm_internal.h word for word.  Two comparators -- bit for bit on
small integers, derived bounds on real values --, the routes' arithmetic restated in numpy with switches that plant
defects, and the graphs ("builders") that reach each route; every builder asserts the census it claims.

Operands are fp64 numpy arrays holding values the element type represents exactly; element types are torch dtypes."""
import numpy as np
import torch

from tests import spmm_forward_reference as fr
from tests.spmm_forward_reference import TINY, U_ACC, U_OUT, store

FLOATS = fr.FLOATS
# exact mode: every sum of an element stays an integer the element type holds (p significant bits: 2^p)
EXACT_LIMIT = {torch.bfloat16: 2.0 ** 8, torch.float16: 2.0 ** 11, torch.float32: 2.0 ** 24, torch.float64: 2.0 ** 53}
K_BW_ROWS, K_BW_SLOTS, K_BW_TILES, MASKED_CHUNK = 2, 512, 2, 8  # kBwRows, kBwSlots, kBwTiles, kMaskedChunk
W_LADDER = (32, 33, 64, 96, 100, 128, 132, 160, 161, 256, 260, 288, 1024, 1056, 1088)
DEFECTS = ('winner_at_cap_lost', 'odd_half_added_to_even', 'zero_mate_replaced', 'bitmap_from_four_words',
           'bitmap_honoured_beyond_32_words', 'walk_stops_at_64', 'blank_last_record_of_rewrite', 'value_as_element_bits',
           'batch1_not_rewritten', 'empty_column_unwritten', 'inf_times_zero', 'tie_to_larger_id')
SENTINEL = 85.0  # what an unwritten output element holds in the restatements (the GPU tests fill with bytes of 85)


def _b3(a, dtype=np.float64):
    a = np.asarray(a, dtype)
    return a[None] if a.ndim == 2 else a


def element_size(dtype):
    return torch.empty(0, dtype=dtype).element_size()


# ---- gradients ---------------------------------------------------------------------------------------------------
def grads_loops(rowptr, col, value, x, gout, arg, has_value):
    """for every (b, m, k) with a = arg[b, m, k] != E:  grad_value[a] += x[b, col[a], k] * g[b, m, k]  (matrices with
    values only) and grad_mat[b, col[a], k] += value[a] * g[b, m, k]  (1 without values).  -> dict: gv, gm (fp64), and per
    element the sum of |terms| (gv_l1, gm_l1) and the number of terms (gv_n, gm_n); gv* are None without values."""
    x3, g3, a3 = _b3(x), _b3(gout), _b3(arg, np.int64)
    (B, N, K), M, E = x3.shape, g3.shape[1], len(col)
    gv, gv_l1, gv_n = np.zeros(E), np.zeros(E), np.zeros(E, np.int64)
    gm, gm_l1, gm_n = np.zeros((B, N, K)), np.zeros((B, N, K)), np.zeros((B, N, K), np.int64)
    for b in range(B):
        for m in range(M):
            for k in range(K):
                a = int(a3[b, m, k])
                if a == E:
                    continue
                g, c = g3[b, m, k], int(col[a])
                if has_value:
                    t = x3[b, c, k] * g
                    gv[a] += t
                    gv_l1[a] += abs(t)
                    gv_n[a] += 1
                t = (value[a] if has_value else 1.0) * g
                gm[b, c, k] += t
                gm_l1[b, c, k] += abs(t)
                gm_n[b, c, k] += 1
    return _pack(x, has_value, gv, gv_l1, gv_n, gm, gm_l1, gm_n)


def _pack(x, has_value, gv, gv_l1, gv_n, gm, gm_l1, gm_n):
    if np.ndim(x) == 2:
        gm, gm_l1, gm_n = gm[0], gm_l1[0], gm_n[0]
    if not has_value:
        gv = gv_l1 = gv_n = None
    return {'gv': gv, 'gv_l1': gv_l1, 'gv_n': gv_n, 'gm': gm, 'gm_l1': gm_l1, 'gm_n': gm_n}


def grads(rowptr, col, value, x, gout, arg, has_value):
    """grads_loops with np.add.at; sums in long double (so that the reference's own error stays 2^-11 of an fp64 bound),
    returned as long double for the sums and fp64 for the masses."""
    x3, g3, a3 = _b3(x), _b3(gout), _b3(arg, np.int64)
    (B, N, K), E = x3.shape, len(col)
    col = np.asarray(col, np.int64)
    wide = np.longdouble
    b, m, k = np.nonzero(a3 != E)
    a = a3[b, m, k]
    g = g3[b, m, k].astype(wide)
    c = col[a] if E > 0 else np.zeros(0, np.int64)
    gv, gv_l1 = np.zeros(E, wide), np.zeros(E, wide)
    gv_n = np.bincount(a, minlength=E).astype(np.int64)[:E] if E > 0 else np.zeros(0, np.int64)
    if has_value:
        t = x3[b, c, k].astype(wide) * g
        np.add.at(gv, a, t)
        np.add.at(gv_l1, a, np.abs(t))
    t = (np.asarray(value, np.float64)[a].astype(wide) if has_value else wide(1.0)) * g
    flat = (b * N + c) * K + k
    gm, gm_l1 = np.zeros(B * N * K, wide), np.zeros(B * N * K, wide)
    np.add.at(gm, flat, t)
    np.add.at(gm_l1, flat, np.abs(t))
    gm_n = np.bincount(flat, minlength=B * N * K).astype(np.int64)
    shape = (B, N, K)
    return _pack(x, has_value, gv, gv_l1.astype(np.float64), gv_n, gm.reshape(shape), gm_l1.reshape(shape).astype(np.float64),
                 gm_n.reshape(shape))


# ---- winner records ----------------------------------------------------------------------------------------------
def record_words(K):
    """-> (W mask words, S words per record)"""
    W = -(-K // 32)
    return W, (W + 3 + 3) & ~3


def defined_words(K):
    """bool [S]: the words of a record the format defines (mask, row id, two value words, and the bitmap where the
    padding leaves word W + 3); the others are padding and hold anything."""
    W, S = record_words(K)
    d = np.zeros(S, bool)
    d[:W + 3] = True
    if (W + 3) % 4 != 0:
        d[W + 3] = True
    return d


def masked_has_z(K):
    """whether the masked sum reads the bitmap: the padding leaves the word and the mask has at most 32 words"""
    W, _ = record_words(K)
    return W <= 32 and (W + 3) % 4 != 0


def records(row, value, arg, K, dtype, has_value):
    """-> uint32 [B, E, S]; padding words are 0 here and never compared."""
    a3 = _b3(arg, np.int64)
    B, E = a3.shape[0], len(row)
    W, S = record_words(K)
    rec = np.zeros((B, E, S), np.uint32)
    b, m, k = np.nonzero(a3 != E)
    np.bitwise_or.at(rec, (b, a3[b, m, k], k // 32), (np.uint32(1) << (k % 32).astype(np.uint32)))
    rec[:, :, W] = np.asarray(row, np.int64).astype(np.uint32)[None]
    v = np.asarray(value, np.float64) if has_value else np.ones(E)
    if dtype == torch.float64:
        bits = np.ascontiguousarray(v, np.float64).view(np.uint64)
        rec[:, :, W + 1] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32)[None]
        rec[:, :, W + 2] = (bits >> np.uint64(32)).astype(np.uint32)[None]
    else:  # the accumulator of f32 / f16 / bf16 is fp32
        rec[:, :, W + 1] = np.ascontiguousarray(v, np.float64).astype(np.float32).view(np.uint32)[None]
    if (W + 3) % 4 != 0:
        rec[:, :, W + 3] = bitmap_of(rec[:, :, :W])
    return rec


def bitmap_of(mask_words, words=32):
    """bit s = (mask word s != 0), s < 32"""
    n = min(mask_words.shape[-1], words)
    z = np.zeros(mask_words.shape[:-1], np.uint32)
    for s in range(n):
        z |= (mask_words[..., s] != 0).astype(np.uint32) << np.uint32(s)
    return z


def mask_bits(rec, K):
    """bool [B, E, K]: the mask of every record"""
    W, _ = record_words(K)
    sh = np.arange(32, dtype=np.uint32)
    bits = ((rec[:, :, :W, None] >> sh) & np.uint32(1)).astype(bool)
    return bits.reshape(rec.shape[0], rec.shape[1], W * 32)[:, :, :K]


def record_values(rec, K, dtype):
    """fp64 [B, E]: the value words read as accumulator bits"""
    W, _ = record_words(K)
    lo, hi = np.ascontiguousarray(rec[:, :, W + 1]), np.ascontiguousarray(rec[:, :, W + 2])
    if dtype == torch.float64:
        return (lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))).view(np.float64)
    return lo.view(np.float32).astype(np.float64)


def decode(rec, K, M):
    """records -> (arg [B, M, K] with E where no record claims the element, the largest number of records that claim
    one element)"""
    B, E, _ = rec.shape
    W, _ = record_words(K)
    b, e, k = np.nonzero(mask_bits(rec, K))
    m = rec[b, e, W].astype(np.int64)
    arg = np.full((B, M, K), E, np.int64)
    arg[b, m, k] = e
    claims = np.zeros((B, M, K), np.int64)
    np.add.at(claims, (b, m, k), 1)
    return arg, int(claims.max()) if claims.size else 0


def record_mismatches(got, want, K):
    """got: int32 / uint32 words of [B, E, S] (a torch tensor or an array); only the defined words are compared"""
    if hasattr(got, 'detach'):
        got = got.detach().cpu().numpy()
    got = np.ascontiguousarray(got).view(np.uint32).reshape(want.shape)
    d = defined_words(K)
    return int((got[:, :, d] != want[:, :, d]).sum())


# ---- comparators -------------------------------------------------------------------------------------------------
def assert_exact_mode(ref, dtype):
    """every sum of |terms| within what the element type holds exactly, so that any order of additions -- rounded to the
    element type after each one, as the packed atomics do -- gives the exact result"""
    lim = EXACT_LIMIT[dtype]
    for key in ('gv_l1', 'gm_l1'):
        if ref[key] is not None and ref[key].size:
            assert float(ref[key].max()) <= lim, (key, float(ref[key].max()), lim)


def exact_mismatches(got, exact, dtype):
    """elements whose bits differ from the exact result stored in `dtype`; none is excluded"""
    return fr.exact_mismatches(got, np.asarray(exact, np.float64), dtype)


def bound_pull_mat(exact, l1, n, dtype):
    """products rounded to T (u l1), summed in the accumulator type in any order ((n + 1) ua l1), rounded once"""
    u, ua = U_OUT[dtype], U_ACC[dtype]
    return u * l1 + (n + 1.0) * ua * l1 + u * np.abs(np.asarray(exact, np.float64)) + TINY[dtype]


def bound_value(exact, l1, dtype, BK):
    """at most B K products and additions in the accumulator type, rounded once"""
    u, ua = U_OUT[dtype], U_ACC[dtype]
    return (2.0 * BK + 2.0) * ua * l1 + u * np.abs(np.asarray(exact, np.float64)) + TINY[dtype]


def bound_scatter_mat(l1, n, dtype):
    """the product and every addition rounded to T, any order"""
    return (n + 2.0) * U_OUT[dtype] * l1 + n * TINY[dtype]


bound_shadow_mat = bound_pull_mat  # fp32 atomics in any order, one narrowing


def violations(got, exact, bound, dtype):
    """-> (elements outside the bound, the largest error / bound); a NaN counts, no element is excluded"""
    g = got.detach().cpu() if hasattr(got, 'detach') else torch.from_numpy(np.asarray(got))
    g = g.numpy().astype(np.longdouble) if g.dtype == torch.float64 else g.double().numpy()
    exact = np.asarray(exact)
    err = np.abs(g.reshape(exact.shape) - exact).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    bad = ~(err <= bound)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0


def value_violations(col, value, x, gout, arg, got, dtype):
    """grad_value `got` for the winners `arg` (whoever computed them) against bound_value, element by element
    -> (elements outside, the largest error / bound)"""
    ref = grads(None, col, value, x, gout, arg, True)
    BK = (1 if np.ndim(x) == 2 else int(np.prod(np.shape(x)[:-2]))) * np.shape(x)[-1]
    return violations(got, ref['gv'], bound_value(ref['gv'], ref['gv_l1'], dtype, BK), dtype)


# ---- cases -------------------------------------------------------------------------------------------------------
class Case:
    """One problem: pattern, operands (fp64 arrays of values `dtype` holds), and -- computed once, on demand -- the
    forward oracle's winners, the gradients and the records."""

    def __init__(self, rowptr, col, N, K, dtype, reduce, value, x, gout, name=''):
        self.rowptr, self.col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
        self.M, self.E, self.N, self.K = len(rowptr) - 1, len(col), N, K
        self.dtype, self.reduce, self.value, self.x, self.gout, self.name = dtype, reduce, value, x, gout, name
        self.has_value = value is not None
        self.B = 1 if np.ndim(x) == 2 else np.shape(x)[0]
        self.row = np.repeat(np.arange(self.M, dtype=np.int64), np.diff(self.rowptr))
        self._fw = self._ref = self._rec = None
        assert self.E == 0 or (self.col.min() >= 0 and self.col.max() < N)

    @property
    def forward(self):
        if self._fw is None:
            out, _, arg = fr.oracle(self.rowptr, self.col, self.value, self.x, self.reduce, self.dtype)
            self._fw = (out, arg)
        return self._fw

    @property
    def arg(self):
        return self.forward[1]

    @property
    def ref(self):
        if self._ref is None:
            self._ref = grads(self.rowptr, self.col, self.value, self.x, self.gout, self.arg, self.has_value)
        return self._ref

    @property
    def rec(self):
        if self._rec is None:
            self._rec = records(self.row, self.value, self.arg, self.K, self.dtype, self.has_value)
        return self._rec

    def csc(self):
        """(colptr, csr2csc) by a stable host sort of the column ids"""
        perm = np.argsort(self.col, kind='stable').astype(np.int64)
        colptr = np.concatenate([[0], np.cumsum(np.bincount(self.col, minlength=self.N))]).astype(np.int64)
        return colptr, perm

    def rel(self):
        """relative position of every winner inside its row, -1 where there is none: [B, M, K]"""
        a3 = _b3(self.arg, np.int64)
        return np.where(a3 != self.E, a3 - self.rowptr[:-1][None, :, None], -1)


def _ints(rng, shape, amax):
    return (rng.integers(1, amax + 1, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float64)


def _reals(rng, shape, dtype):
    return fr.rounded(rng.standard_normal(shape), dtype if dtype != torch.float64 else torch.float32)


def _losers(n, dtype):
    """n distinct magnitudes above 1 that `dtype` holds (consecutive bit patterns from 1.0 on)"""
    if dtype == torch.float16:
        return torch.arange(0x3C01, 0x3C01 + n, dtype=torch.int32).to(torch.int16).view(torch.float16).double().numpy()
    return torch.arange(0x3F81, 0x3F81 + n, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).double().numpy()


def random_case(rowptr, col, N, K, dtype, reduce, has_value, exact, seed, B=None, amax=2, name=''):
    """operands without a plan: small non-zero integers (exact mode; ties abound, the first occurrence wins) or real
    values"""
    rng = np.random.default_rng(seed)
    E, M = len(col), len(rowptr) - 1
    xs, gs = ((N, K), (M, K)) if B is None else ((B, N, K), (B, M, K))
    if exact:
        v = _ints(rng, E, amax) if has_value else None
        x, g = _ints(rng, xs, amax), _ints(rng, gs, amax)
    else:
        v = fr.rounded((rng.random(E) + 0.2) * rng.choice([-1.0, 1.0], E), dtype if dtype != torch.float64 else torch.float32) \
            if has_value else None
        x, g = _reals(rng, xs, dtype), _reals(rng, gs, dtype)
    return Case(rowptr, col, N, K, dtype, reduce, v, x, g, name)


def planted(rowptr, col, K, plan, dtype, reduce='max', has_value=True, exact=True, seed=0, B=None, N=None, hub=None,
            name=''):
    """Operands in which chosen entries win chosen features.  plan: {row: int [K] or [B, K] of positions inside the row
    (-1: no winner -- every product of that feature is NaN), or None for a row of NaN}.  The entries of a planned row
    have columns no other entry names (asserted), so their x is free: losers get distinct negative products, the chosen
    entry a positive one (all negated for min); values of planned rows are positive.  hub = (column, features): x of
    that column beats every planted winner in those features, in every row that names it.  Rows outside the plan keep
    random operands.  The forward oracle decides what actually won; the builders assert their census from it."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    N = int(col.max()) + 1 if N is None else N
    c = random_case(rowptr, col, N, K, dtype, reduce, has_value, exact, seed, B, 1 if exact else 2, name)
    rng = np.random.default_rng(seed + 1)
    x3 = c.x[None] if B is None else c.x
    sgn = -1.0 if reduce == 'min' else 1.0
    wmax = 2 if 2 * K * x3.shape[0] <= EXACT_LIMIT[dtype] else 1  # (an entry may win every feature)
    counts = np.bincount(col, minlength=N)
    hub_col = hub[0] if hub is not None else -1
    for m, win in plan.items():
        s, e = int(rowptr[m]), int(rowptr[m + 1])
        cols = col[s:e]
        own = cols != hub_col
        assert (counts[cols[own]] == 1).all(), 'a planned row shares a column'
        if c.value is not None:
            c.value[s:e] = 1.0 if exact else fr.rounded(0.5 + rng.random(e - s), dtype if dtype != torch.float64 else torch.float32)
        if win is None:
            x3[:, cols[own], :] = np.nan
            continue
        win = np.broadcast_to(np.asarray(win, np.int64), (x3.shape[0], K))
        lose = -sgn * _losers(e - s, dtype)
        for b in range(x3.shape[0]):
            x3[b, cols[own], :] = lose[own][:, None]
            k = np.nonzero(win[b] >= 0)[0]
            wv = rng.integers(1, wmax + 1, len(k)).astype(np.float64) if exact else fr.rounded(0.5 + rng.random(len(k)), dtype if dtype != torch.float64 else torch.float32)
            x3[b, cols[win[b, k]], k] = sgn * wv
            x3[b, cols[own][:, None], np.nonzero(win[b] < 0)[0][None, :]] = np.nan
    if hub is not None:
        x3[:, hub_col, :] = -sgn * 3.0
        x3[:, hub_col, np.asarray(hub[1], np.int64)] = sgn * 3.0
        if c.value is not None:
            c.value[col == hub_col] = 2.0
    return c


# ---- builders ----------------------------------------------------------------------------------------------------
def scatter_lgG(K):
    """lg_groups(K) of csrc/spmm_bw.hip: lanes per row = K rounded up to a power of two, 64 at the most"""
    lpr = 1
    while lpr < min(K, 64):
        lpr *= 2
    return 6 - (lpr.bit_length() - 1)


def build_row_parallel(K, route, dtype, reduce='max', has_value=True, exact=True, seed=0, B=None, hub_rows=120):
    """The scatter / row-parallel kernel at its LDS capacity.  Rows of cap - 1, cap, cap + 1, 2 cap and 2 cap + 1
    entries (cap from the route query), each once with a winner planted at position cap - 1 and once at cap (where the
    row has one), a row of three passes between rows of one pass in the same wave, short and empty rows, a hub column
    named by `hub_rows` rows that wins the last feature of each 4 there (and feature K - 1), and a row count that is no
    multiple of the rows of a wave.  Even K: features (2j, 2j + 1) of a row share their winner for even j and differ for
    odd j; one feature of one row has no winner at all while its mate has."""
    lgG, cap = route['lgG'], route['cap']
    assert lgG == scatter_lgG(K) and cap == (K_BW_SLOTS // K_BW_ROWS) >> lgG
    per_wave = K_BW_ROWS << lgG
    rng = np.random.default_rng(seed)
    lens, plan, want = [], {}, []
    for d in (cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1):
        for rel in (cap - 1, cap):
            if d < 1 or rel >= d or rel < 0:
                continue
            j = np.arange(K)
            # pairs (2j, 2j + 1): the same entry for even j, neighbours of the target for odd j
            win = np.where((j // 2) % 2 == 0, rel, np.where(j % 2 == 0, max(rel - 1, 0), min(rel + 1, d - 1)))
            win[0] = rel
            if K >= 3:
                win[K - 2] = d - 1  # the last entry of the row
            lens += [int(d), 1, 0, 3]  # (rows of one pass behind it)
            plan[len(lens) - 4] = win
            want.append((len(lens) - 4, rel))
    if K >= 2 and K % 2 == 0 and cap >= 2:  # a pair with one winner: feature 1 of a short row has none
        lens.append(2)
        w = np.zeros(K, np.int64)
        w[1] = -1
        plan[len(lens) - 1] = w
        one_sided = len(lens) - 1
    else:
        one_sided = -1
    lens += [int(v) for v in rng.integers(0, 4, 2 * hub_rows)]
    while len(lens) % per_wave == 0 or len(lens) < per_wave + 1:
        lens.append(1)
    M = len(lens)
    # private columns for every entry, in a shuffled order; the hub column is named by one more entry of `hub_rows` rows
    lens = np.asarray(lens, np.int64)
    hubbed = np.zeros(M, bool)
    hubbed[[m for m in range(M) if m not in plan and lens[m] > 0][:hub_rows]] = True
    assert hubbed.sum() == hub_rows
    lens2 = lens + hubbed
    rowptr = np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)
    E = int(rowptr[-1])
    N = E + 7  # columns nobody names: E .. E + 5 and the hub's neighbours
    hub_col = E + 6
    col = rng.permutation(E).astype(np.int64)
    col[rowptr[1:][hubbed] - 1] = hub_col
    hub_feats = sorted(set([K - 1] + [k for k in range(K) if k % 4 == 3]))
    c = planted(rowptr, col, K, plan, dtype, reduce, has_value, exact, seed, B, N, (hub_col, hub_feats),
                name='row_parallel_K%d' % K)
    # census, from the oracle's winners
    rel = c.rel()
    deg = np.diff(rowptr)
    for m, r in want:
        assert (rel[:, m, :] == r).any(), ('no winner at position', r, 'of row', m)
    assert M % per_wave != 0
    waves = [deg[w:w + per_wave] for w in range(0, M, per_wave)]
    if cap >= 1:
        assert any((w > 2 * cap).any() and ((w <= cap) & (w > 0)).any() for w in waves), 'three passes next to one'
    a3 = _b3(c.arg, np.int64)
    hub_wins = int((np.isin(a3, np.nonzero(col == hub_col)[0])).sum())
    assert hub_wins >= hub_rows, hub_wins
    c.census = {'hub_wins': hub_wins, 'passes': int(-(-deg.max() // cap)), 'per_wave': per_wave}
    if K % 2 == 0:
        lo, hi = a3[..., 0::2], a3[..., 1::2]
        c.census.update(pairs_same=int(((lo == hi) & (lo != E)).sum()), pairs_differ=int(((lo != hi) & (lo != E) & (hi != E)).sum()),
                        pairs_one_sided=int(((lo == E) != (hi == E)).sum()))
        assert c.census['pairs_same'] > 0
        if K >= 4:
            assert c.census['pairs_differ'] > 0
        if one_sided >= 0:
            assert c.census['pairs_one_sided'] > 0
    return c


def build_small(N, K, M, dtype, reduce='max', has_value=True, exact=True, seed=0, B=None, deg=3):
    """a few short rows over N columns with repeats (the shadow cases: B N K odd)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, deg + 1, M)
    lens[0] = deg
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, N, int(rowptr[-1])).astype(np.int64)
    return random_case(rowptr, col, N, K, dtype, reduce, has_value, exact, seed, B, 2, 'small')


def tiny_case(K, dtype, reduce='max', has_value=True, exact=True, seed=0, B=None, entries=300, plant_high=False):
    """The W ladder's graph: a few hundred entries in rows of 0 .. 70 entries, E no multiple of 64, an empty first and
    last row, a NaN row.  plant_high: the only winner of one entry sits in the last feature (at or above 1024 for
    K > 1024)."""
    rng = np.random.default_rng(seed)
    lens = [0, 70, 64, 1, 0, 5]
    while sum(lens) < entries:
        lens.append(int(rng.integers(0, 12)))
    if sum(lens) % 64 == 0:
        lens.append(1)
    lens += [2, 0]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    E = int(rowptr[-1])
    col = rng.permutation(E).astype(np.int64)
    plan = {len(lens) - 2: None}
    if plant_high:
        w = np.zeros(K, np.int64)
        w[K - 1] = 3   # entry 3 of the 5-entry row wins the last feature only
        plan[5] = w
    c = planted(rowptr, col, K, plan, dtype, reduce, has_value, exact, seed, B, E + 3, name='tiny_K%d' % K)
    assert E % 64 != 0 and (_b3(c.arg, np.int64)[:, len(lens) - 2] == E).all()
    if plant_high:
        e = int(rowptr[5]) + 3
        assert (np.nonzero(_b3(c.arg, np.int64)[0, 5] == e)[0] == [K - 1]).all()
    return c


LONG_WINNERS = ('none', 'one', 63, 64, 65, 'K')


def build_record_forward(K, route, dtype, reduce='max', has_value=True, exact=True, seed=0, B=None, long_rows=(1025, 3001),
                         long_winners=LONG_WINNERS):
    """The record-writing forward at its thresholds (`route` of tsamd_spmm_route with arg32: items, snap).  Rows of
    snap and snap + 1 entries across a partition boundary (the first is whole, the second cut: asserted with the
    partition restated in numpy); cut rows of 129, 191, 192, 193 and 1024 entries (the whole-row rewrite, 64 entries a
    step); cut rows of `long_rows` entries (blank pieces, then the distinct-winner walk) whose winners are planted: none
    (a NaN row), one entry for every feature, 63 / 64 / 65 distinct entries, K distinct entries -- among them the first
    and the last entry of the row and of a piece."""
    items, snap = route['items'], route['snap']
    g = fr.Rows(items)
    named = {}
    g.add(0, 3)
    g.align(items - snap + 1)
    named['snap'] = g.add(snap)
    g.add(2)
    g.align(items - snap - 1)
    named['snap1'] = g.add(snap + 1)
    g.add(1, 0)
    for d in (129, 191, 192, 193, 1024):
        if g.diag % items + d < items:  # it would fit into the current partition: start it late enough to be cut
            g.align(items - 70)
        named['rewrite%d' % d] = g.add(d)
        g.add(2)
    plan = {}
    for d in long_rows:
        for wn in long_winners:
            g.align(items - 5)  # five entries in the first piece
            m = g.add(d)
            named['long%d_%s' % (d, wn)] = m
            g.add(1)
            if wn == 'none':
                plan[m] = None
                continue
            n = {'one': 1, 'K': K}.get(wn, wn)
            n = min(n, K)
            # positions: the row's first and last entry, the last of the first piece and the first of the second, ...
            pos = [0, d - 1, 4, 5, items + 4, items + 5]
            step = max((d - 10) // max(n, 1), 1)
            pos += [7 + i * step for i in range(n)]
            pos = list(dict.fromkeys(p for p in pos if 0 <= p < d))[:n]
            plan[m] = np.asarray([pos[k % len(pos)] for k in range(K)], np.int64)
    for d in (129, 191, 192, 193, 1024):
        m = named['rewrite%d' % d]
        w = np.asarray([(k * 37) % d for k in range(K)], np.int64)
        w[0], w[K - 1] = 0, d - 1
        plan[m] = w
    rowptr = g.rowptr()
    E = int(rowptr[-1])
    col = np.random.default_rng(seed).permutation(E).astype(np.int64)
    c = planted(rowptr, col, K, plan, dtype, reduce, has_value, exact, seed, B, E + 2, name='record_forward_K%d' % K)
    # census
    table = fr.partition(rowptr, items, snap)
    cuts = fr.census(rowptr, table, items, snap)['runs']
    assert named['snap'] not in cuts and named['snap1'] in cuts, 'snap rows'
    plain = fr.census(rowptr, fr.partition(rowptr, items, 0), items, 0)['runs']
    assert named['snap'] in plain, 'the snap row would be cut without the snap'
    a3 = _b3(c.arg, np.int64)
    c.named, c.distinct = named, {}
    for name, m in named.items():
        if name.startswith('rewrite') or name.startswith('long'):
            assert m in cuts, (name, 'is not cut')
        if name.startswith('long'):
            wn = name.split('_')[1]
            for b in range(a3.shape[0]):
                n = len(np.unique(a3[b, m][a3[b, m] != E]))
                want = {'none': 0, 'one': 1, 'K': min(K, int(name[4:].split('_')[0]))}.get(wn, None)
                want = min(int(wn), K) if want is None else want
                assert n == want, (name, n, want)
            c.distinct[name] = want
    return c


def build_masked_sum(items, K, dtype, reduce='max', has_value=True, exact=True, seed=0, B=None, max_len=None, max_rows=4096):
    """The pull: the TRANSPOSED pattern is build_chains(items) -- hub columns cut into every chain length the fix-up
    branches on, columns with no entry, a cut last column.  Entry j of a column goes to row (j + offset) mod M with
    M = min(the longest column, max_rows): a hub column longer than that names a row several times (duplicates are
    legal; the first of equal products wins).  The second column that has entries loses everywhere (every mask of its
    entries is empty)."""
    colptr, keys = fr.build_chains(items, seed)
    if max_len is not None:
        lens = np.minimum(np.diff(colptr), max_len)
        colptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    lens = np.diff(colptr)
    N, M = len(lens), min(int(lens.max()), max_rows)
    rng = np.random.default_rng(seed)
    off = rng.integers(0, M, N)
    r = np.concatenate([(np.arange(n) + o) % M for n, o in zip(lens, off)]).astype(np.int64)
    cc = np.repeat(np.arange(N, dtype=np.int64), lens)
    order = np.lexsort((cc, r))
    row, col = r[order], cc[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=M))]).astype(np.int64)
    c = random_case(rowptr, col, N, K, dtype, reduce, has_value, exact, seed, B, 1 if exact else 2, 'masked_sum_K%d' % K)
    loser = int(np.nonzero(lens > 0)[0][1])
    x3 = c.x[None] if B is None else c.x
    x3[:, loser, :] = np.nan  # a NaN never wins
    a3 = _b3(c.arg, np.int64)
    assert not np.isin(a3, np.nonzero(col == loser)[0]).any(), 'the losing column won'
    assert (lens == 0).any() and np.array_equal(c.csc()[0], colptr)
    c.keys = keys
    return c


# ---- the routes' arithmetic, restated (switches plant defects) -----------------------------------------------------
def _acc(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def restate_records(c, defect=None, rewrite_rows=(), long_rows=()):
    """the records of the oracle's winners, with a writer's defect planted"""
    rec = c.rec.copy()
    W = record_words(c.K)[0]
    if defect == 'bitmap_from_four_words' and (W + 3) % 4 != 0:
        rec[:, :, W + 3] = bitmap_of(rec[:, :, :W], 4)
    if defect == 'value_as_element_bits' and c.dtype in (torch.bfloat16, torch.float16):
        v = c.value if c.has_value else np.ones(c.E)
        rec[:, :, W + 1] = store(v, c.dtype).view(torch.int16).numpy().astype(np.uint16).astype(np.uint32)[None]
    if defect == 'blank_last_record_of_rewrite':
        for m in rewrite_rows:
            e = int(c.rowptr[m + 1]) - 1
            rec[:, e, :W] = 0
            if (W + 3) % 4 != 0:
                rec[:, e, W + 3] = 0
    if defect in ('walk_stops_at_64', 'batch1_not_rewritten'):
        for m in long_rows:
            s, e = int(c.rowptr[m]), int(c.rowptr[m + 1])
            for b in range(rec.shape[0]):
                if defect == 'batch1_not_rewritten':
                    drop = np.arange(s, e) if b == 1 else np.zeros(0, np.int64)
                else:
                    winners = np.nonzero(rec[b, s:e, :W].any(axis=1))[0] + s
                    drop = winners[64:]
                rec[b, drop, :W] = 0
                if (W + 3) % 4 != 0:
                    rec[b, drop, W + 3] = 0
    return rec


def restate_pull(c, rec, defect=None):
    """grad_mat as the masked sum makes it from records -- round_T(value g) per (entry, won feature), summed per column in
    the accumulator type in CSC order, rounded once; a 32-feature segment whose bitmap bit is clear is skipped where the
    bitmap is read -- and grad_value as the masked SDDMM does: fp32 / fp64 sum over the won features of x g.
    -> (gm, gv or None) as torch tensors of the element type; unwritten elements hold SENTINEL."""
    T, A = c.dtype, _acc(c.dtype)
    K, (W, S) = c.K, record_words(c.K)
    x3, g3 = _b3(c.x), _b3(c.gout)
    B = x3.shape[0]
    bits = mask_bits(rec, K)
    has_z = masked_has_z(K) or (defect == 'bitmap_honoured_beyond_32_words' and (W + 3) % 4 != 0)
    if has_z:
        z = rec[:, :, W + 3]
        seg = (z[:, :, None] >> np.minimum(np.arange(W), 31).astype(np.uint32)) & np.uint32(1)
        if W > 32:
            seg[:, :, 32:] = 0  # (a 32-bit bitmap has no bit for them: the defect skips them)
        bits = bits & np.repeat(seg.astype(bool), 32, axis=2)[:, :, :K]
    vals = record_values(rec, K, T)
    rows = rec[:, :, W].astype(np.int64)
    colptr, perm = c.csc()
    gm = np.zeros((B, c.N, K), A)
    gv = np.zeros(c.E, A)
    for b in range(B):
        g_e = g3[b][rows[b]]                                       # [E, K]
        prod = fr.rounded(vals[b][:, None] * g_e, T) if c.has_value else g_e
        prod = np.where(bits[b], prod, 0.0).astype(A)
        for n in range(c.N):                                        # CSC order, sequential in the accumulator type
            es = perm[colptr[n]:colptr[n + 1]]
            if len(es):
                gm[b, n] = np.cumsum(prod[es], axis=0, dtype=A)[-1]
        xe = x3[b][c.col]
        if defect == 'inf_times_zero':  # the mask multiplied in instead of selected with: 0 * Inf is a NaN
            with np.errstate(invalid='ignore'):
                t = (xe.astype(A) * (g_e * bits[b]).astype(A)).astype(A)
        else:
            t = np.where(bits[b], xe.astype(A) * g_e.astype(A), 0).astype(A)
        gv += np.cumsum(t, axis=1, dtype=A)[:, -1] if K > 0 else 0
    gm_t = torch.from_numpy(gm).to(T)
    if defect == 'empty_column_unwritten':
        gm_t[:, np.diff(colptr) == 0, :] = SENTINEL
    gm_t = gm_t if np.ndim(c.x) == 3 else gm_t[0]
    return gm_t, (torch.from_numpy(gv).to(T) if c.has_value else None)


def restate_scatter(c, arg=None, defect=None, cap=None, shadow=False, seed=0):
    """spmm_minmax_bw_kernel: grad_mat by additions in the element type, one rounding each, in a shuffled order (the
    packed atomics; `shadow`: fp32 additions and one narrowing), grad_value by fp32 / fp64 LDS sums in passes of `cap`
    entries.  arg: the winners to use (the oracle's by default)."""
    T, A = c.dtype, _acc(c.dtype)
    x3, g3 = _b3(c.x), _b3(c.gout)
    a3 = _b3(c.arg if arg is None else arg, np.int64)
    B, N, K, E = x3.shape[0], c.N, c.K, c.E
    narrow = T in (torch.bfloat16, torch.float16) and not shadow
    b, m, k = np.nonzero(a3 != E)
    a = a3[b, m, k]
    g = g3[b, m, k]
    col_a = c.col[a]
    w = c.value[a] if c.has_value else np.ones(len(a))
    prod = fr.rounded(w * g, T) if narrow else (w.astype(A) * g.astype(A)).astype(A)
    flat = (b * N + col_a) * K + k
    if defect == 'odd_half_added_to_even' and K % 2 == 0:
        # the mates of a word share a winner: the even lane adds both halves -- here into its own half
        a_mate = a3[b, m, k ^ 1]
        flat = np.where((a_mate == a) & (k % 2 == 1), flat - 1, flat)
    extra_flat, extra = np.zeros(0, np.int64), np.zeros(0)
    if defect == 'zero_mate_replaced' and K % 2 == 0:
        a_mate = a3[b, m, k ^ 1]
        differ = (a_mate != a) & (a_mate != E)
        w2 = c.value[a_mate[differ]] if c.has_value else np.ones(int(differ.sum()))
        extra = fr.rounded(w2 * g3[b[differ], m[differ], k[differ] ^ 1], T)
        extra_flat = flat[differ] ^ 1   # (the other half of this lane's word gets the mate's value instead of +0)
    flat, prod = np.concatenate([flat, extra_flat]), np.concatenate([prod, extra])
    order = np.random.default_rng(seed).permutation(len(flat))
    gm = np.zeros(B * N * K, np.float64 if narrow else A)
    if narrow:  # one rounding to T per addition: group by target, add in the shuffled order
        srt = order[np.argsort(flat[order], kind='stable')]
        f, p = flat[srt], prod[srt]
        rank = np.arange(len(f)) - np.searchsorted(f, f, side='left')
        for r in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == r
            gm[f[sel]] = fr.rounded(gm[f[sel]] + p[sel], T)
    else:
        np.add.at(gm, flat[order], prod[order].astype(gm.dtype))
    gm_t = torch.from_numpy(gm.reshape(B, N, K)).to(T)
    gm_t = gm_t if np.ndim(c.x) == 3 else gm_t[0]
    gv_t = None
    if c.has_value:
        rel = a - c.rowptr[c.row[a]]
        keep = np.ones(len(a), bool)
        if defect == 'winner_at_cap_lost':
            keep = rel != cap
        t = (x3[b, col_a, k].astype(A) * g.astype(A)).astype(A)
        gv = np.zeros(E, A)
        np.add.at(gv, a[keep], t[keep])
        gv_t = torch.from_numpy(gv).to(T)
    return gm_t, gv_t


def tie_to_larger_id(c):
    """the winners with every tie given to the LAST entry of the row that attains the winning product (defect 12)"""
    x3 = _b3(c.x)
    a3 = _b3(c.arg, np.int64).copy()
    for b in range(a3.shape[0]):
        for m in range(c.M):
            s, e = int(c.rowptr[m]), int(c.rowptr[m + 1])
            if s == e:
                continue
            p = x3[b][c.col[s:e]]
            if c.has_value:
                p = fr.rounded(c.value[s:e, None] * p, c.dtype)
            k = np.nonzero(a3[b, m] != c.E)[0]
            best = p[a3[b, m, k] - s, k]
            last = (e - s - 1) - np.argmax((p[:, k] == best[None])[::-1], axis=0)
            a3[b, m, k] = s + last
    return a3 if np.ndim(c.arg) == 3 else a3[0]
