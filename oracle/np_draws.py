"""numpy restatement of every random draw of the samplers (csrc/sample.hip) -- TEST INFRASTRUCTURE ONLY.

A draw is a pure function of (seed, frontier position i, draw index j, degree) -- plus the keep flags for the temporal
redraw -- so it can be restated bit for bit:

  philox / fmix32 / umul64hi / permute_index     the primitives (csrc/philox.h, csrc/sample.hip)
  sample_draw / ego_draw / temporal_redraw       what tsamd_sample_plan + _draw, tsamd_ego_plan + _draw and
                                                 tsamd_temporal_redraw write
  host_seed, neighbor_seed, ego_seed,            how the operators (csrc/ops_sample.h) derive the seed of a draw from
  hetero_seed, redraw_seed                       torch's CPU generator
  sample_adj_draws / neighbor_draws /            the draw sources the sequential restatements take as `draws=`
  ego_draws / HeteroDraws                        (oracle/np_oracle.py, tests/ego_reference.py)

Every array is uint64 / int64; 32 x 32-bit products are exact in uint64, the 64 x 64 -> high 64 product is built from
32-bit limbs.  Layout of a Philox call: counter = (lo32(c_lo), hi32(c_lo), c2, c3), key = (lo32(seed), hi32(seed)).
docs/design/oracle_parity.md ("random draws") has the table of every draw's counter and tag.
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
GOLDEN64 = 0x9E3779B97F4A7C15
REDRAW_XOR = 0xA5A5A5A55A5A5A5A
TAG_REPLACE, TAG_FLOYD, TAG_FEISTEL, TAG_REDRAW = 0xD4A3, 0xF10D, 0x5A17, 0x7E4D
FLOYD_MAX_DEG = 64

_U = np.uint64
_m32 = _U(M32)
_s32 = _U(32)


def _u64(x):
    """int / int64 / uint64 (scalar or array) -> uint64 array, two's complement."""
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & M64, dtype=np.uint64)
    x = np.asarray(x)
    return x if x.dtype == np.uint64 else x.astype(np.int64).view(np.uint64)


# ---- primitives -----------------------------------------------------------------------------------------------------
def philox(seed, c_lo, c2, c3):
    """Philox4x32-10 (Salmon et al., SC'11): -> (x, y, z, w), uint64 arrays holding 32-bit words."""
    seed = int(seed) & M64
    k0, k1 = seed & M32, seed >> 32
    c_lo = _u64(c_lo)
    x, y = c_lo & _m32, c_lo >> _s32
    z, w = _u64(c2) & _m32, _u64(c3) & _m32
    x, y, z, w = np.broadcast_arrays(x, y, z, w)
    m0, m1 = _U(0xD2511F53), _U(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * x, m1 * z
        x, y, z, w = (p1 >> _s32) ^ y ^ _U(k0), p1 & _m32, (p0 >> _s32) ^ w ^ _U(k1), p0 & _m32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return x, y, z, w


def fmix32(h):
    """MurmurHash3's 32-bit finaliser on uint64 arrays that hold 32-bit words."""
    h = _u64(h) & _m32
    h = h ^ (h >> _U(16))
    h = (h * _U(0x85EBCA6B)) & _m32
    h = h ^ (h >> _U(13))
    h = (h * _U(0xC2B2AE35)) & _m32
    return h ^ (h >> _U(16))


def umul64hi(a, b):
    """High 64 bits of the 128-bit product of two uint64 (arrays)."""
    a, b = _u64(a), _u64(b)
    al, ah, bl, bh = a & _m32, a >> _s32, b & _m32, b >> _s32
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> _s32) + (lh & _m32) + (hl & _m32)
    return hh + (lh >> _s32) + (hl >> _s32) + (mid >> _s32)


def _u01_word(x, y):
    """u64(lo, hi) of sample.hip: the 64-bit uniform word of a Philox output."""
    return x | (y << _s32)


def _bit_length(v):
    """Number of bits of every uint64 in v (0 for 0)."""
    v = _u64(v).copy()
    b = np.zeros(v.shape, dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (v >> _U(s)) != 0
        b = np.where(big, b + _U(s), b)
        v = np.where(big, v >> _U(s), v)
    return b + (v != 0).astype(np.uint64)


def feistel_keys(seed, row):
    """The six round keys of row `row`: (a.x, a.y, a.z, a.w, c.x, c.y) of philox(seed, row, 0 | 1, 0x5A17)."""
    a = philox(seed, row, 0, TAG_FEISTEL)
    c = philox(seed, row, 1, TAG_FEISTEL)
    return (a[0], a[1], a[2], a[3], c[0], c[1])


def permute_index(j, deg, seed, row, rounds=6, keys=None):
    """pi_row(j): the keyed bijection of [0, deg) (balanced Feistel network on 2 * ceil(bits(deg - 1) / 2) bits, cycle
    walking).  j, deg, row broadcast; `rounds` is 6 in the kernels (fewer only for the mutation checks); `keys` may hold
    feistel_keys(seed, row) when the caller has them already."""
    j, deg, row = np.broadcast_arrays(_u64(j), _u64(deg), _u64(row))
    keys = feistel_keys(seed, row) if keys is None else [np.broadcast_to(k, j.shape) for k in keys]
    h = (_bit_length(deg - _U(1)) + _U(1)) >> _U(1)
    hmask = (_U(1) << h) - _U(1)
    fshift = _U(32) - h
    x = j.copy()
    out = np.empty(j.shape, dtype=np.uint64)
    todo = np.arange(j.size)
    xf, outf = x.reshape(-1), out.reshape(-1)
    hf, mf, sf, df = h.reshape(-1), hmask.reshape(-1), fshift.reshape(-1), deg.reshape(-1)
    kf = [np.asarray(k).reshape(-1) for k in keys]
    while todo.size:
        cur, hh, mm, ss = xf[todo], hf[todo], mf[todo], sf[todo]
        L, R = cur >> hh, cur & mm
        for r in range(rounds):
            f = fmix32(((R & _m32) * _U(0x9E3779B1) + kf[r][todo]) & _m32)
            L, R = R, (L ^ (f >> ss)) & mm
        cur = (L << hh) | R
        done = cur < df[todo]
        outf[todo[done]] = cur[done]
        xf[todo] = cur
        todo = todo[~done]
    return out


# ---- the draws of one hop --------------------------------------------------------------------------------------------
def _floyd(seed, i, deg, k, fallback=True):
    """Floyd's k-subset of [0, deg) for every row (arrays i, deg; scalar k < deg <= 64), in emission order: [rows, k].
    fallback=False plants the defect of the mutation checks (pick0 is taken even when it is used already)."""
    used = np.zeros(i.shape, dtype=np.uint64)
    out = np.empty((i.size, k), dtype=np.uint64)
    for c in range(k):
        t = deg - _U(k) + _U(c)
        x, y, _, _ = philox(seed, i, t, TAG_FLOYD)
        pick0 = umul64hi(_u01_word(x, y), t + _U(1))
        taken = ((used >> pick0) & _U(1)) != 0
        pick = np.where(taken, t, pick0) if fallback else pick0
        used = used | (_U(1) << pick)
        out[:, c] = pick
    return out


def _positions(deg, cnt, k, replace, seed, take_all):
    """p[t] of every draw: rows i = 0..F-1 with degree deg[i] contribute cnt[i] draws; take_all[i] marks the rows that
    are listed in stored order.  -> (out_ptr, seg, p)."""
    F = deg.size
    out_ptr = np.zeros(F + 1, dtype=np.int64)
    np.cumsum(cnt, out=out_ptr[1:])
    T = int(out_ptr[-1])
    seg = np.repeat(np.arange(F, dtype=np.int64), cnt)
    j = np.arange(T, dtype=np.int64) - out_ptr[seg]
    p = j.copy()
    if T == 0:
        return out_ptr, seg, p
    d = deg[seg]
    rnd = ~take_all[seg]
    if replace:
        m = rnd
        x, y, _, _ = philox(seed, seg[m], j[m], TAG_REPLACE)
        p[m] = umul64hi(_u01_word(x, y), d[m]).view(np.int64)
    else:
        small = rnd & (d <= FLOYD_MAX_DEG)
        rows = np.nonzero(~take_all & (deg <= FLOYD_MAX_DEG) & (cnt > 0))[0]
        if rows.size:
            picks = _floyd(seed, _u64(rows), _u64(deg[rows]), int(k))
            p[small] = picks.reshape(-1).view(np.int64)
        m = rnd & (d > FLOYD_MAX_DEG)
        if m.any():
            p[m] = permute_index(j[m], d[m], seed, seg[m]).view(np.int64)
    return out_ptr, seg, p


def sample_draw(rowptr, idx, k, replace, seed):
    """tsamd_sample_plan + tsamd_sample_draw (k < 0: tsamd_select_fill, every entry in stored order) for the frontier
    idx -> (out_ptr[F + 1], e_id[T]); nbr = col[e_id].  The draws are keyed by the POSITION in idx, not by the node."""
    rowptr, idx = np.asarray(rowptr, np.int64), np.asarray(idx, np.int64)
    s = rowptr[idx]
    deg = rowptr[idx + 1] - s
    if k < 0:
        cnt, take_all = deg, np.ones(idx.size, bool)
    elif replace:
        cnt, take_all = np.where(deg > 0, k, 0), np.zeros(idx.size, bool)
    else:
        cnt, take_all = np.minimum(deg, k), deg <= k
    out_ptr, seg, p = _positions(deg, cnt.astype(np.int64), k, replace, seed, take_all)
    return out_ptr, s[seg] + p


def ego_draw(rowptr, frontier, k, replace, seed):
    """tsamd_ego_plan + tsamd_ego_draw -> (out_ptr[F + 1], positions[T] in col).  The whole row when deg <= k in both
    replace modes, nothing when k < 0."""
    rowptr, frontier = np.asarray(rowptr, np.int64), np.asarray(frontier, np.int64)
    s = rowptr[frontier]
    deg = rowptr[frontier + 1] - s
    cnt = np.zeros_like(deg) if k < 0 else np.where(deg <= k, deg, k)
    out_ptr, seg, p = _positions(deg, cnt.astype(np.int64), k, replace, seed, deg <= k)
    return out_ptr, s[seg] + p


def temporal_redraw(out_ptr, k, seed, keep, last_valid=True):
    """tsamd_temporal_redraw: k uniform picks per frontier node among its listed draws with keep = 1, in stored order
    -> (t[F * k], keep2[F * k]): draw x = i * k + j copies listed draw t[x] (0 and keep2 = 0 for a node without one).
    `seed` is the seed the kernel receives (redraw_seed of the draw's seed).  last_valid=False plants the defect of the
    mutation checks (the picks index [0, cnt - 1))."""
    out_ptr, keep = np.asarray(out_ptr, np.int64), np.asarray(keep, np.int64)
    F = out_ptr.size - 1
    rank = np.zeros(keep.size + 1, dtype=np.int64)
    np.cumsum(keep, out=rank[1:])
    order = np.nonzero(keep)[0]
    i = np.repeat(np.arange(F, dtype=np.int64), k)
    j = np.tile(np.arange(k, dtype=np.int64), F)
    lo = rank[out_ptr[i]]
    cnt = rank[out_ptr[i + 1]] - lo
    keep2 = (cnt > 0).astype(np.int64)
    x, y, _, _ = philox(seed, i, j, TAG_REDRAW)
    span = cnt if last_valid else np.maximum(cnt - 1, 1)
    pick = umul64hi(_u01_word(x, y), np.maximum(span, 0)).view(np.int64)
    t = np.zeros(F * k, dtype=np.int64)
    has = cnt > 0
    t[has] = order[(lo + pick)[has]]
    return t, keep2


# ---- seeds ------------------------------------------------------------------------------------------------------------
def host_seed(s):
    """The 64-bit seed an operator draws from torch's CPU generator right after torch.manual_seed(s).  The caller seeds
    again before it calls the operator."""
    import torch
    torch.manual_seed(s)
    return int(torch.randint(0, 2**63 - 1, (1, )))


def neighbor_seed(seed0, hop):
    """neighbor_sample: the seed of hop `hop` (0-based)."""
    return (seed0 + GOLDEN64 * (hop + 1)) & M64


ego_seed = neighbor_seed  # ego_k_hop_sample_adj derives its hop seeds the same way


def hetero_seed(seed0, draw_no):
    """hetero samplers: draw_no counts every (hop, relation in sorted key order) from 1, empty frontiers included."""
    return (seed0 + GOLDEN64 * draw_no) & M64


def redraw_seed(seed):
    return (seed ^ REDRAW_XOR) & M64


# ---- draw sources for the sequential restatements -----------------------------------------------------------------------
def sample_adj_draws(seed0, replace):
    """sample_adj: one draw, keyed by seed0 itself -> draws(hop, rowptr, frontier, k) = (out_ptr, positions)."""
    return lambda hop, rowptr, frontier, k: sample_draw(rowptr, frontier, k, replace, seed0)


def neighbor_draws(seed0, replace):
    return lambda hop, colptr, frontier, k: sample_draw(colptr, frontier, k, replace, neighbor_seed(seed0, hop))


def ego_draws(seed0, replace):
    return lambda hop, rowptr, frontier, k: ego_draw(rowptr, frontier, k, replace, ego_seed(seed0, hop))


class HeteroDraws:
    """Draw source of hetero_neighbor_sample / hetero_temporal_neighbor_sample."""

    def __init__(self, seed0, replace):
        self.seed0, self.replace = seed0, replace

    def sample(self, draw_no, colptr, frontier, k, replace=None):
        replace = self.replace if replace is None else replace
        return sample_draw(colptr, frontier, k, replace, hetero_seed(self.seed0, draw_no))

    def redraw(self, draw_no, out_ptr, keep, k):
        return temporal_redraw(out_ptr, k, redraw_seed(hetero_seed(self.seed0, draw_no)), keep)
