"""Sampled hot-row side table of the SpMM forward (docs/design/spmm_forward.md, "Hot rows"): sums and means of one
matrix whose column ids camp copy only the rows that a sample of `col` hits; the merge kernel gathers those from the
side table and the others in place.  Only addresses change, so every case is checked against the oracle AND bit for
bit against the same call with the operand cache switched on, which takes the full relabelled copy.  That the route
was taken at all is read from the workspace (tsamd_spmm_hot_rows_layout): flags, and the table's rows, after a call."""
import ctypes

import pytest
import torch

from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd import synth
from tests.util import bits_equal, check_spmm

pytestmark = pytest.mark.gpu

N, M, E = 9001, 5000, 1300000  # n is no multiple of 64: the last lookup word is partial


@pytest.fixture(scope='module')
def ops():
    import pytorch_sparse_amd  # noqa: F401
    return torch.ops


@pytest.fixture(autouse=True)
def _cache_off(ops):
    ops.tsamd.operand_cache(False)
    yield
    ops.tsamd.operand_cache(False)


def _skewed(n=N, m=M, e=E, seed=11):
    g = torch.Generator().manual_seed(seed)
    row, col = torch.randint(0, m, (e, ), generator=g), torch.randint(0, n, (e, ), generator=g)
    col[::3] &= ~7  # low-bit skew, as the probe looks for
    return row, col


def _csr(row, col, m):
    """CSR of the entries as they are (duplicates stay: E is the stated size), rows in order."""
    order = torch.argsort(row, stable=True)
    rp = torch.zeros(m + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(row, minlength=m), 0)
    return rp, col[order].contiguous()


def _features(n, K, dtype, seed=0):
    return synth.features(n, K, seed=seed).to(dtype)


def _both_ways(ops, dev, rp, c, v, x, reduces=('sum', 'mean')):
    rp, c, x = rp.to(dev), c.to(dev), x.to(dev)
    v = None if v is None else v.to(dev)
    for reduce in reduces:
        def call():
            if reduce == 'sum':
                return ops.torch_sparse.spmm_sum(None, rp, c, v, None, None, x)
            return ops.torch_sparse.spmm_mean(None, rp, c, v, None, None, None, x)
        ops.tsamd.operand_cache(False)
        out = call()
        check_spmm(out, None, rp, c, v, x, reduce)
        ops.tsamd.operand_cache(True)
        full = call()  # fills the cache: the full relabelled copy
        ops.tsamd.operand_cache(False)
        assert bits_equal(out, full), 'hot-row table and full copy differ (%s)' % reduce


SENTINEL = 0xAB


def _inspect(dev, rp, c, v, x):
    """tsamd_spmm (sum) on a workspace of our own, filled with a sentinel byte -> (out, flags [N] uint8, table rows
    [H, K] as the call left them, or None when the library says the call keeps the full copy)."""
    rp, c, x = rp.to(dev), c.to(dev), x.to(dev)
    v = None if v is None else v.to(dev)
    L = nat.lib()
    i64 = ctypes.c_int64
    dt, red = nat.dtype_code(x.dtype), nat.REDUCES['sum']
    m, e, (n, K) = rp.numel() - 1, c.numel(), x.shape
    dims = (i64(1), i64(m), i64(n), i64(K), i64(e))
    out = torch.empty(m, K, dtype=x.dtype, device=dev)
    ws = torch.full((L.tsamd_spmm_workspace_bytes(dt, red, *dims), ), SENTINEL, dtype=torch.uint8, device=dev)
    lay = (ctypes.c_int64 * 4)()
    hot = L.tsamd_spmm_hot_rows_layout(dt, red, *dims, nat._ptr(x), nat._ptr(out), nat._ptr(ws), lay)
    with torch.cuda.device(dev):
        st = L.tsamd_spmm(dt, red, nat._ptr(rp), nat._ptr(c), nat._ptr(v), nat._ptr(x), nat._ptr(out), nat._ptr(None),
                          *dims, nat._ptr(ws), ctypes.c_size_t(ws.numel()), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_spmm')
    torch.cuda.synchronize()
    if not hot:
        return out, None, None
    flags = ws[lay[0]:lay[0] + n].clone()
    row_bytes = K * x.element_size()
    assert (ws.data_ptr() + lay[2] - x.data_ptr()) == lay[3] * row_bytes, 'the table is a whole number of rows from mat'
    table = ws[lay[2]:lay[2] + n * row_bytes].view(n, row_bytes)
    return out, flags, table


def _check_hot(dev, ops, rp, c, v, x, must_be_hot=()):
    """The hot route was taken: some ids are flagged, only ids that `col` names, `must_be_hot` among them; the table
    holds exactly their rows, in id order, and nothing behind them; the result equals the op's bit for bit."""
    out, flags, table = _inspect(dev, rp, c, v, x)
    assert flags is not None, 'the call kept the full copy'
    named = torch.zeros(x.shape[0], dtype=torch.bool, device=dev)
    named[c.to(dev)] = True
    hot = flags == 1
    assert bool(((flags == 0) | hot).all()) and int(hot.sum()) > 0 and bool((named | ~hot).all())
    for i in must_be_hot:
        assert bool(hot[i]), 'id %d is gathered 200 k times and not in the table' % i
    H = int(hot.sum())
    want = x.to(dev).contiguous().view(torch.uint8).view(x.shape[0], -1)[hot]
    assert torch.equal(table[:H], want), 'table rows differ from the hot rows of mat'
    assert bool((table[H:] == SENTINEL).all()), 'rows written behind the last slot'
    full = ops.torch_sparse.spmm_sum(None, rp.to(dev), c.to(dev), None if v is None else v.to(dev), None, None, x.to(dev))
    assert bits_equal(out, full)
    return H


def test_common_shape(dev, ops):
    row, col = _skewed()
    rp, c = _csr(row, col, M)
    v, x = synth.values(E, seed=1) - 0.3, _features(N, 64, torch.float32)
    _both_ways(ops, dev, rp, c, v, x)
    _check_hot(dev, ops, rp, c, v, x)


def test_two_hubs_first_and_last_id(dev, ops):
    """Ids 0 and n - 1 with 200 k entries each over a cold skewed remainder: hot and cold gathers meet in one window."""
    row, col = _skewed(seed=12)
    g = torch.Generator().manual_seed(5)
    pos = torch.randperm(E, generator=g)[:400000]
    col[pos[:200000]] = 0
    col[pos[200000:]] = N - 1
    rp, c = _csr(row, col, M)
    v, x = synth.values(E, seed=2) - 0.3, _features(N, 64, torch.float32, seed=1)
    _both_ways(ops, dev, rp, c, v, x)
    H = _check_hot(dev, ops, rp, c, v, x, must_be_hot=(0, N - 1))
    assert H < N, 'some ids stay cold: hot and cold gathers meet'


def test_every_column_hot(dev, ops):
    """n = 4096, E = 2^20 (the smallest shape that takes the copy): the first 4096 of the entries at multiples of 128 walk
    through all ids, the other 4096 hold multiples of 8, so a sample of every 8th, 32nd or 128th entry hits every id
    while the probe (it reads multiples of 64) still sees the low-bit skew.  The table fills to capacity."""
    n, m, e = 4096, 2048, 1 << 20
    g = torch.Generator().manual_seed(13)
    col = torch.randint(0, n, (e, ), generator=g)
    col[::3] &= ~7
    j = torch.arange(e // 128)
    col[::128] = torch.where(j < n, j, (j * 8) % n)
    rp = torch.arange(m + 1, dtype=torch.int64) * (e // m)
    v, x = synth.values(e, seed=3) - 0.3, _features(n, 64, torch.float32, seed=2)
    _both_ways(ops, dev, rp, col, v, x)
    assert _check_hot(dev, ops, rp, col, v, x) == n


def test_mat_16_bytes_into_its_storage(dev, ops):
    row, col = _skewed(seed=14)
    rp, c = _csr(row, col, M)
    buf = torch.empty(N * 64 + 4, device=dev)
    x = buf[4:].view(N, 64)
    x.copy_(_features(N, 64, torch.float32, seed=3))
    assert x.data_ptr() % 256 == 16 and x.is_contiguous()
    _both_ways(ops, dev, rp, c, None, x, reduces=('sum', ))
    _check_hot(dev, ops, rp, c, None, x)


@pytest.mark.parametrize('dtype', [torch.float64, torch.bfloat16])
def test_other_types_at_256_byte_rows(dev, ops, dtype):
    row, col = _skewed(seed=15)
    rp, c = _csr(row, col, M)
    K = 256 // torch.empty(0, dtype=dtype).element_size()
    v = (synth.values(E, seed=4) - 0.3).to(dtype)
    x = _features(N, K, dtype, seed=4)
    _both_ways(ops, dev, rp, c, v, x, reduces=('sum', ))
    _check_hot(dev, ops, rp, c, v, x)


def test_uniform_graph_copies_nothing(dev, ops):
    """Uniform ids: the probe does not fire and every prologue kernel leaves at once.  Read from the workspace: the call
    is in scope (the layout exists), the flag array was cleared and no id marked, and not one byte of the table's
    region was written.  By `profile=` stage times: the prologue of the uniform graph, idle launches only, is no longer
    than that of the skewed graph of the same shape, which runs the same launches and marks, ranks and copies on top;
    20 us are allowed for the resolution of a median of 9 event timings of ~40-us stages."""
    g = torch.Generator().manual_seed(16)
    row, col = torch.randint(0, M, (E, ), generator=g), torch.randint(0, N, (E, ), generator=g)
    rp, c = _csr(row, col, M)
    v, x = synth.values(E, seed=5) - 0.3, _features(N, 64, torch.float32, seed=5)
    _both_ways(ops, dev, rp, c, v, x)
    out, flags, table = _inspect(dev, rp, c, v, x)
    assert flags is not None and int(flags.sum()) == 0, 'an id was marked on a graph the probe does not flag'
    assert bool((table == SENTINEL).all()), 'rows were copied'
    srow, scol = _skewed(seed=17)
    srp, sc = _csr(srow, scol, M)

    def prologue(rp_, c_):
        a = (rp_.to(dev), c_.to(dev), v.to(dev), x.to(dev))
        times = []
        for _ in range(11):
            p = []
            nat.spmm(*a, 'sum', profile=p)
            times.append(p[0])
        return sorted(times[2:])[4]
    uni, skew = prologue(rp, c), prologue(srp, sc)
    print('prologue: uniform graph %.3f ms, skewed graph of the same shape %.3f ms (medians of 9)' % (uni, skew))
    assert uni <= skew + 0.02
