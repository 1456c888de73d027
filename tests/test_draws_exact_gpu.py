"""Every random draw of the samplers, bit for bit against oracle/np_draws.py (whose law tests/test_draw_oracle.py
pins on the CPU): the draw kernels through the C ABI (include/tsamd.h) at the degrees and fan-outs where they branch,
and the whole operators under torch.manual_seed against the sequential restatements with np_draws as their draw source.

Tie rule (stated once): a row of the R-MAT graph may hold the same column twice; sample_adj sorts every row by the new
column id and may order the e_id of such equal columns either way (so may the reference's std::sort).  e_id is
therefore compared through the column it points to, plus the sorted e_id of every row; everything else is
assert_array_equal on the arrays themselves."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import np_draws as npd
from oracle import np_oracle as npo

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SEEDS = (0, 2**64 - 1, 0x1234567890ABCDEF)
DEGREES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1001, 4096, 4097, 2**16 + 1, 2**20 + 1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
I = lambda x: ctypes.c_int64(int(x))  # noqa: E731


@pytest.fixture(scope='module')
def nat():
    from pytorch_sparse_amd import _native
    L = _native.lib()
    for name in ('tsamd_sample_workspace_bytes', 'tsamd_ego_plan_workspace_bytes', 'tsamd_temporal_redraw_workspace_bytes'):
        getattr(L, name).restype = ctypes.c_size_t
    return _native


@pytest.fixture(scope='module')
def rows():
    """One row per degree class (both sides of the take-all, Floyd and Feistel boundaries and of every change of the
    Feistel half width up to 2^20 + 1); the columns are node ids of the same graph."""
    deg = np.asarray(DEGREES, np.int64)
    rowptr = np.zeros(deg.size + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = np.random.default_rng(0).integers(0, deg.size, int(rowptr[-1]))
    return rowptr, col, dev(rowptr), dev(col)


def _empty(n):
    return torch.full((int(n), ), -1, dtype=torch.long, device=DEV)


def gpu_sample(nat, rp, c, idx, k, replace, seed):
    """tsamd_sample_plan + tsamd_sample_draw -> (out_ptr, e_id, nbr) as numpy"""
    L, st = nat.lib(), nat.stream_ptr(rp.device)
    n, M = idx.numel(), rp.numel() - 1
    out_ptr, info = _empty(n + 1), _empty(2)
    ws = nat.workspace(L.tsamd_sample_workspace_bytes(I(n)), rp.device)
    nat.check(L.tsamd_sample_plan(P(rp), I(M), P(idx), I(n), I(k), ctypes.c_int(replace), P(out_ptr), P(info), P(ws),
                                  ctypes.c_size_t(ws.numel()), st), 'plan')
    T, bad = info.tolist()
    assert bad == 0
    e_id, nbr = _empty(T), _empty(T)
    nat.check(L.tsamd_sample_draw(P(rp), P(c), P(idx), I(n), I(k), ctypes.c_int(replace), ctypes.c_uint64(seed), P(out_ptr),
                                  P(e_id), P(nbr), st), 'draw')
    return host(out_ptr), host(e_id), host(nbr)


@pytest.mark.parametrize('replace', [0, 1])
@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 1000])
def test_sample_draw_matches_the_oracle_at_every_branch(nat, rows, k, replace):
    """idx lists every row three times (the key of a draw is the position in idx, not the node).  Includes deg = 65 with
    k = 64 (64 Feistel draws) and deg = 1001 with k = 1000 (all positions but one: the missing one must be the
    oracle's)."""
    rowptr, col, rp, c = rows
    idx = np.concatenate([np.arange(len(DEGREES)), np.arange(len(DEGREES))[::-1], np.arange(len(DEGREES))])
    for seed in SEEDS:
        out_ptr, e_id, nbr = gpu_sample(nat, rp, c, dev(idx), k, replace, seed)
        want_ptr, want_e = npd.sample_draw(rowptr, idx, k, bool(replace), seed)
        np.testing.assert_array_equal(out_ptr, want_ptr)
        np.testing.assert_array_equal(e_id, want_e)
        np.testing.assert_array_equal(nbr, col[want_e])


def test_sample_draw_all_but_one_entry_of_the_longest_row(nat, rows):
    """deg = 2^20 + 1 with k = 2^20: the bijection evaluated at all positions but one."""
    rowptr, col, rp, c = rows
    idx = np.asarray([DEGREES.index(1001), DEGREES.index(2**20 + 1)])
    out_ptr, e_id, nbr = gpu_sample(nat, rp, c, dev(idx), 2**20, 0, SEEDS[2])
    want_ptr, want_e = npd.sample_draw(rowptr, idx, 2**20, False, SEEDS[2])
    np.testing.assert_array_equal(out_ptr, want_ptr)
    np.testing.assert_array_equal(e_id, want_e)
    np.testing.assert_array_equal(nbr, col[want_e])
    assert np.unique(e_id).size == e_id.size == 1001 + 2**20


def gpu_ego(nat, rp, c, frontier, fseg, k, replace, seed):
    L, st = nat.lib(), nat.stream_ptr(rp.device)
    F, M = frontier.numel(), rp.numel() - 1
    out_ptr, words = _empty(F + 1), torch.zeros(2, dtype=torch.long, device=DEV)
    ws = nat.workspace(L.tsamd_ego_plan_workspace_bytes(I(F)), rp.device)
    total, err = ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(words.data_ptr() + 8)
    nat.check(L.tsamd_ego_plan(P(rp), I(M), P(frontier), I(F), I(k), P(out_ptr), total, err, P(ws),
                               ctypes.c_size_t(ws.numel()), st), 'ego_plan')
    T = int(words[0])
    nbr, seg = _empty(T), _empty(T)
    nat.check(L.tsamd_ego_draw(P(rp), P(c), I(M), P(frontier), P(fseg), I(F), I(k), ctypes.c_int(replace),
                               ctypes.c_uint64(seed), P(out_ptr), I(T), P(nbr), P(seg), err, st), 'ego_draw')
    assert int(words[1]) == 0
    return host(out_ptr), host(nbr), host(seg)


@pytest.mark.parametrize('replace', [0, 1])
@pytest.mark.parametrize('k', [1, 3, 64, 1000, 2**20 + 2])
def test_ego_draw_matches_the_oracle_over_empty_segments(nat, rows, k, replace):
    """The same rows as a frontier with zero-degree entries first, last and in runs between the others (the segment
    search of a draw has to step over empty segments); a frontier of one entry; k = 1 and k above every degree."""
    rowptr, col, rp, c = rows
    z = DEGREES.index(0)
    order = [z, z] + [x for r in range(1, len(DEGREES)) for x in ((r, z, z, z) if r % 3 == 0 else (r, ))] + [z]
    big = DEGREES.index(2**20 + 1)
    if k > 2**20:  # every row whole: keep the hub to one entry
        order = [x for x in order if x != big] + [big, z]
    for frontier in (np.asarray(order), np.asarray([DEGREES.index(129)])):
        fseg = np.arange(frontier.size) // 2
        for seed in SEEDS[1:]:
            out_ptr, nbr, seg = gpu_ego(nat, rp, c, dev(frontier), dev(fseg), k, replace, seed)
            want_ptr, want_pos = npd.ego_draw(rowptr, frontier, k, bool(replace), seed)
            np.testing.assert_array_equal(out_ptr, want_ptr)
            np.testing.assert_array_equal(nbr, col[want_pos])
            np.testing.assert_array_equal(seg, np.repeat(fseg, np.diff(want_ptr)))


@pytest.mark.parametrize('k', [1, 3, 7])
@pytest.mark.parametrize('F', [1, 255, 256, 257])
def test_temporal_mark_and_redraw_match_the_oracle(nat, F, k):
    """F * k on both sides of the 256-thread block; neighbour lists of 0, 1 and 40 entries; valid sets none / only the
    first / only the last / all: keep (tsamd_temporal_mark) and nbr2, e2, seg2, keep2 (tsamd_temporal_redraw)."""
    L, st = nat.lib(), nat.stream_ptr(torch.device(DEV, 0))
    rng = np.random.default_rng(F * 10 + k)
    i = np.arange(F)
    length = np.asarray([40, 1, 0])[i % 3] if F > 1 else np.asarray([40])
    out_ptr = np.zeros(F + 1, np.int64)
    np.cumsum(length, out=out_ptr[1:])
    T = int(out_ptr[-1])
    seg = np.repeat(i, length)
    j = np.arange(T) - out_ptr[seg]
    pattern = (i // 3 + (F == 1) * k) % 4  # 0 none, 1 only the first, 2 only the last, 3 all
    want_keep = np.select([pattern[seg] == 0, pattern[seg] == 1, pattern[seg] == 2], [0, j == 0, j == length[seg] - 1], 1)
    want_keep = want_keep.astype(np.int64)
    nbr = rng.permutation(T)  # one source node per listed draw
    src_time = np.empty(T, np.int64)
    src_time[nbr] = np.where(want_keep > 0, rng.integers(0, 6, T), rng.integers(6, 12, T))
    f_time = np.full(F, 5, np.int64)
    e = rng.integers(0, 10**6, T)
    d_nbr, d_seg, d_e, d_src_time, d_f_time = dev(nbr), dev(seg), dev(e), dev(src_time), dev(f_time)
    keep = _empty(T)
    nat.check(L.tsamd_temporal_mark(P(d_nbr), P(d_seg), I(T), P(d_src_time), P(d_f_time), P(keep), st), 'mark')
    np.testing.assert_array_equal(host(keep), want_keep)
    free = _empty(T)
    nat.check(L.tsamd_temporal_mark(P(d_nbr), P(d_seg), I(T), None, None, P(free), st), 'mark')
    np.testing.assert_array_equal(host(free), np.ones(T, np.int64))
    ws = nat.workspace(L.tsamd_temporal_redraw_workspace_bytes(I(T)), keep.device)
    d_ptr = dev(out_ptr)
    for seed in SEEDS[1:]:
        for flags, d_flags in ((want_keep, keep), (np.ones(T, np.int64), free)):
            out = [_empty(F * k) for _ in range(4)]
            nat.check(L.tsamd_temporal_redraw(P(d_ptr), I(F), I(T), I(k), ctypes.c_uint64(seed), P(d_nbr), P(d_e), P(d_flags),
                                              P(out[0]), P(out[1]), P(out[2]), P(out[3]), P(ws), ctypes.c_size_t(ws.numel()),
                                              st), 'redraw')
            t, keep2 = npd.temporal_redraw(out_ptr, k, seed, flags)
            np.testing.assert_array_equal(host(out[3]), keep2, err_msg='keep2')
            np.testing.assert_array_equal(host(out[0]), np.where(keep2 > 0, nbr[t], 0), err_msg='nbr2')
            np.testing.assert_array_equal(host(out[1]), np.where(keep2 > 0, e[t], 0), err_msg='e2')
            np.testing.assert_array_equal(host(out[2]), np.repeat(i, k), err_msg='seg2')


# ---- whole operators under torch.manual_seed -------------------------------------------------------------------------
@pytest.fixture(scope='module')
def big():
    import pytorch_sparse_amd  # noqa: F401
    from pytorch_sparse_amd import synth
    rowptr, col = synth.rmat_csr(17, 16, seed=5)  # the `big` graph of tests/test_sample_gpu.py: every degree class
    rowptr, col = rowptr.numpy(), col.numpy()
    return rowptr, col, dev(rowptr), dev(col)


@pytest.mark.parametrize('replace', [False, True])
@pytest.mark.parametrize('k', [1, 5, 25])
def test_sample_adj_matches_the_oracle(big, k, replace):
    rowptr, col, rp, c = big
    idx = np.random.default_rng(k).permutation(rowptr.size - 1)[:30_000]
    seed0 = npd.host_seed(100 + k)
    torch.manual_seed(100 + k)
    got = [host(t) for t in torch.ops.torch_sparse.sample_adj(rp, c, dev(idx), k, replace)]
    want = npo.sample_adj_all(rowptr, col, idx, k, npd.sample_adj_draws(seed0, replace))
    for g, w, key in zip(got[:3], want[:3], ('rowptr', 'col', 'n_id')):
        np.testing.assert_array_equal(g, w, err_msg=key)
    np.testing.assert_array_equal(col[got[3]], col[want[3]])  # the tie rule of the module docstring
    seg = np.repeat(np.arange(idx.size), np.diff(want[0]))
    np.testing.assert_array_equal(got[3][np.lexsort((got[3], seg))], want[3][np.lexsort((want[3], seg))])


@pytest.mark.parametrize('replace', [False, True])
def test_neighbor_sample_matches_the_oracle(big, replace):
    colptr, row, cp, rw = big  # the CSR arrays used as a CSC: same structure
    inp = np.random.default_rng(2).permutation(colptr.size - 1)[:1024]
    fan = [10, 5, 3]
    seed0 = npd.host_seed(7)
    for directed in (True, False):
        torch.manual_seed(7)
        got = torch.ops.torch_sparse.neighbor_sample(cp, rw, dev(inp), fan, replace, directed)
        want = npo.neighbor_sample(colptr, row, inp, fan, directed, npd.neighbor_draws(seed0, replace))
        for g, w, key in zip(got, want, ('node', 'row', 'col', 'edge')):
            np.testing.assert_array_equal(host(g), w, err_msg='%s directed=%s' % (key, directed))


NODE_TYPES = ['paper', 'author', 'venue']
EDGE_TYPES = [('author', 'writes', 'paper'), ('paper', 'cites', 'paper'), ('paper', 'in', 'venue'),
              ('venue', 'hosts', 'paper'), ('paper', 'by', 'author')]
RELS = ['__'.join(e) for e in EDGE_TYPES]


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_hetero_samplers_match_the_oracle(seed):
    """The random graphs of test_random_graphs_against_the_sequential_restatement with fan-outs BELOW the degrees:
    both replace modes, 1 to 3 hops, directed / undirected / temporal, one relation emptied and one type without times
    (odd seeds), input nodes listed twice.  A few tens of thousands of draws through the sequential Python oracle."""
    import pytorch_sparse_amd  # noqa: F401
    ops = torch.ops.torch_sparse
    rng = np.random.default_rng(100 + seed)
    sizes = {'paper': int(rng.integers(50, 3000)), 'author': int(rng.integers(20, 1000)), 'venue': int(rng.integers(2, 40))}
    colptr, row = {}, {}
    for (s, r, d) in EDGE_TYPES:
        deg = rng.integers(0, 9, sizes[d])
        deg[::3] = 0
        cp = np.zeros(sizes[d] + 1, np.int64)
        np.cumsum(deg, out=cp[1:])
        colptr['__'.join((s, r, d))] = cp
        row['__'.join((s, r, d))] = rng.integers(0, sizes[s], int(cp[-1]))
    if seed % 2:
        colptr['venue__hosts__paper'] = np.zeros_like(colptr['venue__hosts__paper'])
        row['venue__hosts__paper'] = row['venue__hosts__paper'][:0]
    times = {t: rng.integers(0, 30, sizes[t]) for t in NODE_TYPES}
    seeds = rng.integers(0, sizes['paper'], 40)
    seeds[7], seeds[21] = seeds[3], seeds[3]
    inp = {'paper': seeds, 'author': rng.integers(0, sizes['author'], 5)}
    D = lambda d: {k: dev(v) for k, v in d.items()}  # noqa: E731
    C, R, In = D(colptr), D(row), D(inp)
    tm = {t: v for t, v in times.items() if t != 'venue'} if seed % 2 else times
    Tm = D(tm)

    def compare(got, want, what):
        for t in NODE_TYPES:
            np.testing.assert_array_equal(host(got[0][t]), want[0][t], err_msg='%s node %s' % (what, t))
        for r in RELS:
            for x in (1, 2, 3):
                np.testing.assert_array_equal(host(got[x][r]), want[x][r], err_msg='%s %s %d' % (what, r, x))

    for hops in (1, 2, 3):
        fan = {r: [3, 2, 4][:hops] for r in RELS}
        for replace in (False, True):
            s = 1000 * seed + 10 * hops + replace
            draws = npd.HeteroDraws(npd.host_seed(s), replace)
            for directed in (True, False):
                torch.manual_seed(s)
                got = ops.hetero_neighbor_sample(NODE_TYPES, EDGE_TYPES, C, R, In, fan, hops, replace, directed)
                want = npo.hetero_neighbor_sample_det(NODE_TYPES, EDGE_TYPES, colptr, row, inp, fan, hops, directed,
                                                      replace=replace, draws=draws)
                compare(got, want, 'hops=%d replace=%s directed=%s' % (hops, replace, directed))
            torch.manual_seed(s)
            got = ops.hetero_temporal_neighbor_sample(NODE_TYPES, EDGE_TYPES, C, R, In, fan, Tm, hops, replace, True)
            want = npo.hetero_neighbor_sample_det(NODE_TYPES, EDGE_TYPES, colptr, row, inp, fan, hops, True, tm,
                                                  replace=replace, draws=draws)
            compare(got, want, 'temporal hops=%d replace=%s' % (hops, replace))


@pytest.mark.parametrize('replace', [False, True])
@pytest.mark.parametrize('k', [1, 3])
def test_ego_k_hop_sample_adj_matches_the_oracle(k, replace):
    """Depth 1 to 3 on a graph with rows below and above the Floyd boundary, seeds listed twice: all six outputs."""
    import pytorch_sparse_amd  # noqa: F401
    from tests.ego_reference import ego_assemble, ego_node_sets
    rng = np.random.default_rng(4)
    n = 400
    deg = rng.integers(0, 9, n)
    deg[::7] = 0
    deg[5], deg[6] = 70, 130
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1]))
    col[rng.integers(0, col.size, 60)] = rng.choice([5, 6], 60)  # the long rows are reached
    idx = rng.integers(0, n, 24)
    idx[3], idx[9], idx[10] = 5, idx[0], idx[0]
    for depth in (1, 2, 3):
        s = 10 * depth + k
        seed0 = npd.host_seed(s)
        torch.manual_seed(s)
        got = torch.ops.torch_sparse.ego_k_hop_sample_adj(dev(rowptr), dev(col), dev(idx), depth, k, replace)
        sets = ego_node_sets(rowptr, col, idx, depth, k, npd.ego_draws(seed0, replace))
        want = ego_assemble(rowptr, col, idx, sets)
        for g, w, key in zip(got, want, ('rowptr', 'col', 'n_id', 'e_id', 'ptr', 'root_n_id')):
            np.testing.assert_array_equal(host(g), w, err_msg='%s depth=%d' % (key, depth))
