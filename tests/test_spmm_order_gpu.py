"""Column order of the SpMM merge kernel (docs/design/spmm_forward.md, "Column order"): the slot -> partition map that
the prologue builds on the device must equal the numpy restatement (tests/spmm_order_reference.py) word for word, and
the output with the order forced on must equal the output with it off bit for bit -- only the order of execution
changes.  Header, keys and map are read from a sentinel-filled workspace after a call (tsamd_spmm_order_layout)."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd import synth
from tests import spmm_order_reference as R
from tests.util import bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SENTINEL32 = 0xA5A5A5A5


@pytest.fixture(autouse=True)
def _auto_again():
    nat.lib().tsamd_spmm_column_order(1)
    yield
    nat.lib().tsamd_spmm_column_order(1)


def graph(M, hubs, N=None, seed=0, low=0, high=8):
    """rows of low..high-1 entries plus hub rows {row: entries}; column ids sorted inside a row"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(low, high, size=M)
    for r, n in hubs.items():
        deg[r] = n
    N = N or max(M, int(deg.max()) + 1)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(N, size=int(d), replace=False)) for d in deg] + [np.zeros(0, dtype=np.int64)])
    return torch.from_numpy(rowptr), torch.from_numpy(col.astype(np.int64)), N


def run(dev, rp, c, v, x, reduce, setting):
    """tsamd_spmm on a sentinel-filled workspace under tsamd_spmm_column_order(setting) -> (out, layout or None, ws)"""
    L = nat.lib()
    i64 = ctypes.c_int64
    assert L.tsamd_spmm_column_order(setting) == setting
    dt, red = nat.dtype_code(x.dtype), nat.REDUCES[reduce]
    M, E = rp.numel() - 1, c.numel()
    N, K = x.shape[-2], x.shape[-1]
    B = x.numel() // (N * K)
    dims = (i64(B), i64(M), i64(N), i64(K), i64(E))
    out = torch.empty(list(x.shape[:-2]) + [M, K], dtype=x.dtype, device=dev)
    arg = torch.empty(out.shape, dtype=torch.int64, device=dev) if red >= 2 else None
    ws = torch.full((L.tsamd_spmm_workspace_bytes(dt, red, *dims), ), SENTINEL, dtype=torch.uint8, device=dev)
    lay = nat.spmm_order_layout(x.dtype, reduce, B, M, N, K, E, x, out, ws)
    with torch.cuda.device(dev):
        st = L.tsamd_spmm(dt, red, nat._ptr(rp), nat._ptr(c), nat._ptr(v), nat._ptr(x), nat._ptr(out), nat._ptr(arg), *dims,
                          nat._ptr(ws), ctypes.c_size_t(ws.numel()), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_spmm')
    torch.cuda.synchronize()
    return out, lay, ws


def words(ws, off, n):
    return ws[off:off + 4 * n].cpu().numpy().view(np.uint32).astype(np.int64)


def expected(rp, c, x, reduce):
    """numpy: (single, key, P) of the call's own partition (P and items from tsamd_spmm_route)"""
    M, E = rp.numel() - 1, c.numel()
    N, K = x.shape[-2], x.shape[-1]
    B = x.numel() // (N * K)
    route = nat.spmm_route(x.dtype, reduce, B, M, N, K, E)
    table = R.partition_table(rp.numpy(), E, route['items'], route['P'])
    single, key = R.classify(rp.numpy(), c.numpy(), table)
    return single, key, route


def check_forced(dev, rp, c, x, v=None, want_singles=None):
    """forced on: header, keys and map equal numpy; sum and mean equal the call with the order off, bit for bit"""
    single, key, route = expected(rp, c, x, 'sum')
    if want_singles is not None:
        assert want_singles(int(single.sum()), route['P']), (int(single.sum()), route['P'])
    rpd, cd, xd = rp.to(dev), c.to(dev), x.to(dev)
    vd = None if v is None else v.to(dev)
    for reduce in ('sum', 'mean'):
        off, lay0, _ = run(dev, rpd, cd, vd, xd, reduce, 0)
        assert lay0 is None
        on, lay, ws = run(dev, rpd, cd, vd, xd, reduce, 2)
        assert lay is not None and lay['mode'] == 2 and lay['P'] == route['P']
        hdr = words(ws, lay['hdr_off'], 3)
        assert hdr[0] == 1 and hdr[1] == int(single.sum())
        assert np.array_equal(words(ws, lay['keys_off'], route['P']), key)
        got = words(ws, lay['order_off'], route['P'])
        R.check_order(got, single, key)
        assert np.array_equal(got, R.slot_map(single, key))
        assert bits_equal(on, off), 'column order changed the result (%s)' % reduce
    return route


def feats(N, K, B=1, seed=1):
    x = synth.features(B * N, K, seed=seed)
    return x.view(B, N, K) if B > 1 else x


def test_two_single_row_partitions(dev):
    """a few hundred short rows behind one row of 3 x items + 1 entries: exactly two single-row partitions"""
    it = 128
    rp, c, N = graph(300, {0: 3 * it + 1})
    route = check_forced(dev, rp, c, feats(N, 64), want_singles=lambda s, P: s == 2)
    assert route['items'] == it


def test_fewer_than_eight(dev):
    """fewer single-row partitions than a wave has lanes, than there are XCDs"""
    rp, c, N = graph(300, {17: 6 * 128})
    check_forced(dev, rp, c, feats(N, 64), want_singles=lambda s, P: 0 < s < 8)


def test_one_row(dev):
    """M = 1: every partition but the ends is single-row"""
    rp, c, N = graph(1, {0: 5000})
    check_forced(dev, rp, c, feats(N, 64), v=synth.values(5000), want_singles=lambda s, P: s == P - 2)


PCOUNT_ROWS = [299, 301, 317, 340]


def _pcount_graph(M):
    return graph(M, {5: 9000, 40: 7001, M - 1: 4000}, seed=M)


@pytest.mark.parametrize('M', PCOUNT_ROWS)
def test_partition_counts(dev, M):
    """P not a multiple of 4, of 8, of 32 (the shapes differ in their number of short rows)"""
    rp, c, N = _pcount_graph(M)
    check_forced(dev, rp, c, feats(N, 64), want_singles=lambda s, P: s > 32)


def test_partition_counts_cover_the_remainders():
    ps = []
    for M in PCOUNT_ROWS:
        rp, c, N = _pcount_graph(M)
        ps.append(nat.spmm_route(torch.float32, 'sum', 1, M, N, 64, c.numel())['P'])
    assert any(p % 4 for p in ps) and any(p % 8 for p in ps) and any(p % 32 for p in ps), ps


@pytest.mark.parametrize('K', [64, 260])
def test_feature_tiles(dev, K):
    """ktiles 1 and 2 (gridDim.y > 1)"""
    rp, c, N = graph(500, {3: 20000, 250: 9000})
    route = check_forced(dev, rp, c, feats(N, K), v=synth.values(c.numel()), want_singles=lambda s, P: s > 8)
    assert route['ktiles'] == (1 if K == 64 else 2)


def test_two_matrices(dev):
    rp, c, N = graph(500, {3: 20000, 250: 9000})
    route = check_forced(dev, rp, c, feats(N, 64, B=2), want_singles=lambda s, P: s > 8)
    assert route['grid_y'] == 2


def test_ties_go_to_the_smaller_partition(dev):
    """a hub row that names two ids only: long runs of equal keys, in one bucket"""
    deg = torch.tensor([3] * 10 + [6000] + [2] * 20)
    rp = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    c = torch.cat([torch.arange(3).repeat(10), torch.tensor([7] * 3100 + [4000] * 2900), torch.arange(2).repeat(20)])
    N = 4096
    single, key, _ = expected(rp, c, feats(N, 64), 'sum')
    k = key[single]
    assert k.size > 40 and np.unique(k).size <= 3
    check_forced(dev, rp, c, feats(N, 64))


@pytest.fixture(scope='module')
def big_uniform():
    """in auto's scope (E = 2^20, N = 8192 = E / 128) and without a single-row partition: rows of 128 entries"""
    M = N = 8192
    rp = torch.arange(M + 1, dtype=torch.int64) * 128
    g = torch.Generator().manual_seed(3)
    c = torch.randint(0, N, (M, 128), generator=g).sort(dim=1)[0].reshape(-1)
    return rp, c, N


@pytest.fixture(scope='module')
def big_skewed():
    """in auto's scope (E >= 2^20, E >= 8 N) with most entries in rows longer than a partition"""
    return graph(4096, {r: 8192 + 2 * r for r in range(0, 4096, 41)}, N=16384, seed=5, low=0, high=16)


def test_auto_idles_on_a_uniform_graph(dev, big_uniform):
    rp, c, N = big_uniform
    x = feats(N, 64)
    single, key, route = expected(rp, c, x, 'sum')
    assert int(single.sum()) == 0
    off, _, _ = run(dev, rp.to(dev), c.to(dev), None, x.to(dev), 'sum', 0)
    out, lay, ws = run(dev, rp.to(dev), c.to(dev), None, x.to(dev), 'sum', 1)
    assert lay is not None and lay['mode'] == 1
    hdr = words(ws, lay['hdr_off'], 3)
    assert hdr[0] == 0 and hdr[1] == 0
    assert np.all(words(ws, lay['order_off'], lay['P']) == SENTINEL32), 'the builder wrote a map nobody reads'
    assert bits_equal(out, off)


def test_auto_engages_on_a_skewed_graph(dev, big_skewed):
    """the default setting, through the C-ABI (the header says that it engaged) and through torch.ops"""
    import pytorch_sparse_amd  # noqa: F401
    rp, c, N = big_skewed
    x = feats(N, 64)
    single, key, route = expected(rp, c, x, 'sum')
    assert c.numel() >= 1 << 20 and c.numel() >= 8 * N
    assert int(single.sum()) >= 1024 and 8 * int(single.sum()) >= route['P']
    rpd, cd, xd = rp.to(dev), c.to(dev), x.to(dev)
    assert nat.lib().tsamd_spmm_column_order(-1) == 1
    out, lay, ws = run(dev, rpd, cd, None, xd, 'sum', 1)
    assert lay is not None and lay['mode'] == 1
    hdr = words(ws, lay['hdr_off'], 3)
    assert hdr[0] == 1 and hdr[1] == int(single.sum())
    assert np.array_equal(words(ws, lay['order_off'], lay['P']), R.slot_map(single, key))
    via_op = torch.ops.torch_sparse.spmm_sum(None, rpd, cd, None, None, None, xd)
    assert torch.ops.tsamd.column_order(0) == 0
    plain = torch.ops.torch_sparse.spmm_sum(None, rpd, cd, None, None, None, xd)
    assert torch.ops.tsamd.column_order(1) == 1
    assert bits_equal(out, plain) and bits_equal(via_op, plain)


def test_excluded_families_keep_identity_order(dev):
    """min / max, short rows, the partial product and the record-writing forward: no order, forced or not, and the same
    results"""
    rp, c, N = graph(500, {3: 20000, 250: 9000})
    x = feats(N, 64)
    rpd, cd, xd = rp.to(dev), c.to(dev), x.to(dev)
    for reduce in ('max', 'min'):
        off, _, _ = run(dev, rpd, cd, None, xd, reduce, 0)
        on, lay, _ = run(dev, rpd, cd, None, xd, reduce, 2)
        assert lay is None and bits_equal(on, off)
    x16 = feats(N, 16).to(dev)  # rows of 64 bytes: the side-by-side kernel
    off, _, _ = run(dev, rpd, cd, None, x16, 'sum', 0)
    on, lay, _ = run(dev, rpd, cd, None, x16, 'sum', 2)
    assert lay is None and bits_equal(on, off)
    outs = []
    for setting in (0, 2):
        assert nat.lib().tsamd_spmm_column_order(setting) == setting
        o = torch.zeros(500, 64, device=dev)
        nat.spmm_partial(rpd, cd, None, xd, 'sum', o, accumulate=True)
        outs.append(o)
    assert bits_equal(outs[0], outs[1])
    # the record-writing forward (128 features: the 32-byte records)
    row, x128, recs = nat.ptr2ind(rpd, cd.numel()), feats(N, 128).to(dev), []
    for setting in (0, 2):
        assert nat.lib().tsamd_spmm_column_order(setting) == setting
        recs.append(nat.spmm_minmax_records(rpd, cd, None, x128, 'max', row, zero=True))
    assert bits_equal(recs[0][0], recs[1][0]) and torch.equal(recs[0][1], recs[1][1])
