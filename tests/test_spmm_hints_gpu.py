"""Pattern hints of the SpMM forward (docs/design/spmm_forward.md, "Pattern hints"): what the prologue derives from
(rowptr, col) alone is built once per pattern and reused.  The hints are advisory, so every case compares with the
stateless tsamd_spmm BIT FOR BIT: reuse with the same pattern, reuse after the pattern was overwritten in place behind
torch's back, and -- through the C-ABI -- hints that were built from another graph altogether.  The cache of the torch
ops is read through its control op, torch.ops.tsamd.pattern_hints() -> [entries, builds, reuses], which also drops
every entry: a case reads it once, at its end.

The graphs: N = M = 65536, K = 64 fp32 (256-byte rows), the smallest shape of the hot-block route.  48 hub rows of 8192
entries over the multiples of 8 (the probe flags the graph; every hub row is 64 partitions of 128 items, 63 of them
single-row: the column order engages), 11 entries in every other row, 80 % of them in every fourth 64-id block (those
blocks are selected).  The uniform graph has the same M, N and E, is not flagged and has no single-row partition."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd import synth
from tests.util import bits_equal

pytestmark = pytest.mark.gpu

N = M = 65536
K = 64
HUBS, HUB_LEN, SHORT = 48, 8192, 11
E = HUBS * HUB_LEN + (M - HUBS) * SHORT
SENTINEL = 0xA5


def hub_graph(seed):
    g = torch.Generator().manual_seed(seed)
    hubs = torch.randperm(M, generator=g)[:HUBS]
    deg = torch.full((M, ), SHORT, dtype=torch.int64)
    deg[hubs] = HUB_LEN
    rp = torch.zeros(M + 1, dtype=torch.int64)
    rp[1:] = deg.cumsum(0)
    anyid = torch.randint(0, N, (E, ), generator=g)
    pop_blocks = torch.arange(seed % 4, N // 64, 4)
    pop = pop_blocks[torch.randint(0, pop_blocks.numel(), (E, ), generator=g)] * 64 + torch.randint(0, 64, (E, ), generator=g)
    col = torch.where(torch.rand(E, generator=g) < 0.8, pop, anyid)
    for h in hubs.tolist():
        col[rp[h]:rp[h + 1]] = torch.arange(HUB_LEN) * 8
    return rp, col


def uniform_graph(seed):
    g = torch.Generator().manual_seed(seed)
    deg = torch.full((M, ), E // M, dtype=torch.int64)
    deg[:E - (E // M) * M] += 1
    rp = torch.zeros(M + 1, dtype=torch.int64)
    rp[1:] = deg.cumsum(0)
    return rp, torch.randint(0, N, (E, ), generator=g)


@pytest.fixture(scope='module')
def ops():
    import pytorch_sparse_amd  # noqa: F401
    return torch.ops


@pytest.fixture(scope='module')
def data(dev):
    """patterns (0 - 4 hub graphs, 'u' the uniform one), values, four X, and the stateless results, computed once"""
    pats = {i: tuple(t.to(dev) for t in hub_graph(i)) for i in range(5)}
    pats['u'] = tuple(t.to(dev) for t in uniform_graph(9))
    v = (synth.values(E, seed=1) - 0.3).to(dev)
    xs = [synth.features(N, K, seed=10 + i).to(dev) for i in range(4)]
    refs = {}

    def ref(p, i, reduce='sum'):
        if (p, i, reduce) not in refs:
            refs[(p, i, reduce)] = nat.spmm(pats[p][0], pats[p][1], v, xs[i], reduce)[0]
        return refs[(p, i, reduce)]
    return pats, v, xs, ref


@pytest.fixture(autouse=True)
def _fresh(ops):
    nat.lib().tsamd_spmm_column_order(1)
    ops.tsamd.operand_cache(False)
    ops.tsamd.pattern_hints()
    yield
    ops.tsamd.pattern_hints()


def spmm_sum(ops, rp, c, v, x):
    return ops.torch_sparse.spmm_sum(None, rp, c, v, None, None, x)


def counters(ops, since=(0, 0, 0)):
    n, b, r = ops.tsamd.pattern_hints()
    return n, b - since[1], r - since[2]


def words(buf, off, n):
    return buf[off:off + 4 * n].cpu().numpy().view(np.uint32).astype(np.int64)


def test_both_routes_are_taken(dev, data):
    """the route and layout queries say so, and hints built through the C-ABI hold both verdicts"""
    pats, v, xs, ref = data
    rp, c = pats[0]
    assert E >= 1 << 20 and E >= 8 * N
    ws = nat.workspace(nat.lib().tsamd_spmm_workspace_bytes(0, 0, *(ctypes.c_int64(s) for s in (1, M, N, K, E))), dev)
    out = torch.empty(M, K, device=dev)
    assert nat.spmm_route(torch.float32, 'sum', 1, M, N, K, E, mat=xs[0], out=out, workspace=ws)['family'] == 'hot_blocks'
    order = nat.spmm_order_layout(torch.float32, 'sum', 1, M, N, K, E, xs[0], out, ws)
    assert order is not None and order['mode'] == 1
    lay = nat.spmm_hints_layout(torch.float32, 'sum', 1, M, N, K, E)
    assert lay['P'] == order['P']
    hints = torch.full((lay['bytes'], ), SENTINEL, dtype=torch.uint8, device=dev)
    built = nat.spmm_hinted(rp, c, v, xs[0], 'sum', hints, 1)
    assert bits_equal(built, ref(0, 0))
    f = words(hints, lay['flags_off'], 4)
    assert f[3] >= 4096 and f[1] * 4 > f[3], 'the probe flags the graph'
    hdr = words(hints, lay['hdr_off'], 3)
    assert hdr[0] == 1 and hdr[1] >= 1024 and 8 * hdr[1] >= lay['P'], 'the column order engages'
    bw = words(hints, lay['words_off'], N // 64)
    sel = int((bw != 0).sum())
    assert 0 < sel < N // 64 and sorted(bw[bw != 0]) == list(range(1, sel + 1)), 'some blocks selected: ranks 1 .. S'
    assert int(words(hints, lay['totals_off'], 128).sum()) == sel
    assert sorted(words(hints, lay['order_off'], lay['P'])) == list(range(lay['P'])), 'a permutation of the partitions'
    # the uniform graph: neither verdict
    rpu, cu = pats['u']
    hints.fill_(SENTINEL)
    assert bits_equal(nat.spmm_hinted(rpu, cu, v, xs[0], 'sum', hints, 1), ref('u', 0))
    f = words(hints, lay['flags_off'], 4)
    assert f[3] >= 4096 and f[1] * 4 <= f[3] and f[2] * 16 <= f[3]
    assert words(hints, lay['hdr_off'], 2).tolist() == [0, 0]


def test_a_reuse_call_runs_no_pattern_only_kernel(dev, data):
    """state 2 on a sentinel-filled workspace: the probe's counters, the flag bytes and the keys of the classification
    are never written there, and the hints do not change"""
    pats, v, xs, ref = data
    rp, c = pats[1]
    lay = nat.spmm_hints_layout(torch.float32, 'sum', 1, M, N, K, E)
    hints = torch.empty(lay['bytes'], dtype=torch.uint8, device=dev)
    nat.spmm_hinted(rp, c, v, xs[0], 'sum', hints, 1)
    before = hints.clone()
    L = nat.lib()
    dims = tuple(ctypes.c_int64(s) for s in (1, M, N, K, E))
    ws = torch.full((L.tsamd_spmm_workspace_bytes(0, 0, *dims), ), SENTINEL, dtype=torch.uint8, device=dev)
    out = nat.spmm_hinted(rp, c, v, xs[1], 'sum', hints, 2, ws=ws)
    assert bits_equal(out, ref(1, 1))
    assert torch.equal(hints, before)
    route = nat.spmm_route(torch.float32, 'sum', 1, M, N, K, E, mat=xs[1], out=out, workspace=ws)
    hot = (ctypes.c_int64 * 4)()
    assert L.tsamd_spmm_hot_blocks_layout(0, 0, *dims, nat._ptr(xs[1]), nat._ptr(out), nat._ptr(ws), hot) == 1
    order = nat.spmm_order_layout(torch.float32, 'sum', 1, M, N, K, E, xs[1], out, ws)
    for name, off, n in [('probe counters', route['relabel_flag_off'], 16), ('flag bytes', hot[0], N),
                         ('block words', hot[1], 4 * (N // 64)), ('order header', order['hdr_off'], 12),
                         ('keys', order['keys_off'], 4 * order['P']), ('map', order['order_off'], 4 * order['P'])]:
        assert bool((ws[off:off + n] == SENTINEL).all()), name + ' written in a reuse call'
    assert not bool((ws[route['table_off']:route['table_off'] + 16 * (route['P'] + 1)] == SENTINEL).all()), 'the table is rebuilt'


def test_reuse_is_bit_identical(ops, data):
    pats, v, xs, ref = data
    rp, c = pats[0]
    c0 = ops.tsamd.pattern_hints()
    for i in range(3):
        assert bits_equal(spmm_sum(ops, rp, c, v, xs[i]), ref(0, i)), 'call %d' % i
    mean = ops.torch_sparse.spmm_mean(None, rp, c, v, None, None, None, xs[3])
    assert bits_equal(mean, ref(0, 3, 'mean'))
    assert counters(ops, c0) == (1, 1, 3), 'one build, then reuses'


@pytest.mark.parametrize('first,then', [(0, 'u'), ('u', 0), (0, 1)])
def test_stale_hints_cannot_change_a_result(dev, ops, data, first, then):
    """reuse established on one graph, then rowptr / col overwritten in place through .data (no version bump): the
    stale hints are reused and the result is the stateless result of the new graph in every bit"""
    pats, v, xs, ref = data
    rp, c = pats[first][0].clone(), pats[first][1].clone()
    c0 = ops.tsamd.pattern_hints()
    assert bits_equal(spmm_sum(ops, rp, c, v, xs[0]), ref(first, 0))
    assert bits_equal(spmm_sum(ops, rp, c, v, xs[1]), ref(first, 1))
    versions = (rp._version, c._version)
    c.data.copy_(pats[then][1])
    rp.data.copy_(pats[then][0])
    assert (rp._version, c._version) == versions
    out = spmm_sum(ops, rp, c, v, xs[2])
    assert counters(ops, c0) == (1, 1, 2), 'the third call reused the stale hints'
    assert bits_equal(out, ref(then, 2))


@pytest.mark.parametrize('built_from,run_on', [(0, 'u'), ('u', 0), (0, 1), (1, 0)])
def test_adversarial_hints_through_the_cabi(dev, data, built_from, run_on):
    pats, v, xs, ref = data
    hints = torch.empty(nat.spmm_hints_bytes(torch.float32, 'sum', 1, M, N, K, E), dtype=torch.uint8, device=dev)
    assert bits_equal(nat.spmm_hinted(*pats[built_from], v, xs[0], 'sum', hints, 1), ref(built_from, 0))
    assert bits_equal(nat.spmm_hinted(*pats[run_on], v, xs[1], 'sum', hints, 2), ref(run_on, 1))
    assert bits_equal(nat.spmm_hinted(*pats[run_on], v, xs[3], 'mean', hints, 2), ref(run_on, 3, 'mean'))


def _established(ops, data):
    pats, v, xs, ref = data
    rp, c = pats[2][0].clone(), pats[2][1].clone()
    c0 = ops.tsamd.pattern_hints()
    for i in range(2):
        assert bits_equal(spmm_sum(ops, rp, c, v, xs[i]), ref(2, i))
    return rp, c, c0


def test_key_another_stream(dev, ops, data):
    pats, v, xs, ref = data
    rp, c, c0 = _established(ops, data)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = spmm_sum(ops, rp, c, v, xs[2])
    torch.cuda.current_stream().wait_stream(s)
    assert bits_equal(out, ref(2, 2))
    assert counters(ops, c0) == (2, 2, 1), 'an entry of its own for the other stream'


def test_key_capturing_stream(dev, ops, data):
    pats, v, xs, ref = data
    rp, c, c0 = _established(ops, data)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = spmm_sum(ops, rp, c, v, xs[2])
    g.replay()
    torch.cuda.synchronize()
    assert bits_equal(out, ref(2, 2))
    assert counters(ops, c0) == (1, 1, 1), 'a capturing stream goes without'


def test_key_version_bump(dev, ops, data):
    pats, v, xs, ref = data
    rp, c, c0 = _established(ops, data)
    c.add_(0)
    assert bits_equal(spmm_sum(ops, rp, c, v, xs[2]), ref(2, 2))
    assert bits_equal(spmm_sum(ops, rp, c, v, xs[3]), ref(2, 3))
    assert counters(ops, c0) == (1, 2, 2), 'built anew in place, then reused'


def test_key_row_bytes(dev, ops, data):
    pats, v, xs, ref = data
    rp, c, c0 = _established(ops, data)
    x128 = synth.features(N, 128, seed=20).to(dev)
    assert bits_equal(spmm_sum(ops, rp, c, v, x128), nat.spmm(rp, c, v, x128, 'sum')[0])
    assert counters(ops, c0) == (2, 2, 1)


def test_key_inference_tensor(dev, ops, data):
    pats, v, xs, ref = data
    rp, c, c0 = _established(ops, data)
    with torch.inference_mode():
        c_inf = c.clone()
        assert c_inf.is_inference()
        out = spmm_sum(ops, rp, c_inf, v, xs[2]).clone()
    assert bits_equal(out, ref(2, 2))
    assert counters(ops, c0) == (1, 1, 1), 'an inference tensor goes without'


def test_eviction(dev, ops, data):
    """five patterns in rotation over four entries: every call builds, results stay equal, and the entries' memory comes
    back when they are dropped; three patterns in rotation are reused"""
    pats, v, xs, ref = data
    for p in range(5):
        ref(p, 0)
    torch.cuda.synchronize()
    c0 = ops.tsamd.pattern_hints()
    base = torch.cuda.memory_allocated()
    for _ in range(2):
        for p in range(5):
            out = spmm_sum(ops, pats[p][0], pats[p][1], v, xs[0])
            assert bits_equal(out, ref(p, 0)), 'pattern %d' % p
            del out
    n, b, r = counters(ops, c0)
    assert (n, b, r) == (4, 10, 0)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base
    c0 = (0, b + c0[1], r + c0[2])
    for _ in range(2):
        for p in range(3):
            assert bits_equal(spmm_sum(ops, pats[p][0], pats[p][1], v, xs[0]), ref(p, 0))
    assert counters(ops, c0) == (3, 3, 3)


def test_out_of_scope_calls_leave_the_counters(dev, ops, data):
    pats, v, xs, ref = data
    c0 = ops.tsamd.pattern_hints()
    assert nat.spmm_hints_bytes(torch.float32, 'sum', 1, 5000, 9001, K, 1300000) == 0
    assert nat.spmm_hints_bytes(torch.float32, 'max', 1, M, N, K, E) == 0
    assert nat.spmm_hints_bytes(torch.float32, 'sum', 2, M, N, K, E) == 0
    rp, c = pats[3]
    for _ in range(2):
        got = ops.torch_sparse.spmm_max(rp, c, v, xs[0])[0]
        assert bits_equal(got, nat.spmm(rp, c, v, xs[0], 'max')[0])
        x2 = torch.stack([xs[0], xs[1]])
        assert bits_equal(spmm_sum(ops, rp, c, v, x2), nat.spmm(rp, c, v, x2, 'sum')[0])
    g = torch.Generator().manual_seed(34)
    n, m, e = 9001, 5000, 1300000
    cs = torch.randint(0, n, (e, ), generator=g).to(dev)
    rps = torch.zeros(m + 1, dtype=torch.int64)
    rps[1:] = torch.cumsum(torch.bincount(torch.randint(0, m, (e, ), generator=g), minlength=m), 0)
    rps, xsmall = rps.to(dev), synth.features(n, K, seed=4).to(dev)
    for _ in range(2):
        assert bits_equal(spmm_sum(ops, rps, cs, None, xsmall), nat.spmm(rps, cs, None, xsmall, 'sum')[0])
    assert counters(ops, c0) == (0, 0, 0)
