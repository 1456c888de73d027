"""Hot blocks of the SpMM forward (docs/design/spmm_forward.md, "Hot blocks"): from N = 65536 on the unit of the side
table is the block of 64 consecutive ids.  A block is selected when at least tsamd_spmm_hot_block_min() of its ids were
flagged by the 1/32 sample of `col`; it gets the 64 table rows of its rank among the selected blocks, rotated inside that
span, and one 4-byte word (rank + 1, or 0).  Only addresses change, so every case is checked against the oracle AND bit for
bit against the same call with the operand cache switched on, which takes the full relabelled copy.  Flags, block words
and table are read from a sentinel-filled workspace after a call (tsamd_spmm_hot_blocks_layout).

The probe reads col[::128] at E = 2^21 and the sample col[::32], and the graphs below are given as CSR directly (rows
of E / M entries), so what is flagged is set by construction where a case needs it."""
import ctypes

import pytest
import torch

from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd import synth
from tests.util import bits_equal, check_spmm

pytestmark = pytest.mark.gpu

N, M, E = 65536 + 41, 8192, 1 << 21  # the last block of 64 ids is partial (41 ids)
WORDS = (N + 63) // 64
SENTINEL = 0xAB


@pytest.fixture(scope='module')
def ops():
    import pytorch_sparse_amd  # noqa: F401
    return torch.ops


@pytest.fixture(autouse=True)
def _cache_off(ops):
    ops.tsamd.operand_cache(False)
    yield
    ops.tsamd.operand_cache(False)


def _kmin():
    return int(nat.lib().tsamd_spmm_hot_block_min())


def _rowptr(m=M, e=E):
    return torch.arange(m + 1, dtype=torch.int64) * (e // m)


def _skewed(seed, popular_every=3):
    """Low-bit skew as the probe looks for, and blocks of unequal popularity: 80 % of the entries name ids of every
    `popular_every`-th block, the others any id -- some blocks reach the threshold and some do not."""
    g = torch.Generator().manual_seed(seed)
    anyid = torch.randint(0, N, (E, ), generator=g)
    pop_blocks = torch.arange(0, WORDS - 1, popular_every)
    pop = pop_blocks[torch.randint(0, pop_blocks.numel(), (E, ), generator=g)] * 64 + torch.randint(0, 64, (E, ), generator=g)
    col = torch.where(torch.rand(E, generator=g) < 0.8, pop, anyid)
    col[::3] &= ~7
    return col


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
        assert bits_equal(out, full), 'block table and full copy differ (%s)' % reduce


def _hooks(dev, rp, c, x):
    """(per-id hook's answer, block hook's answer, block layout, workspace, out) for a sum of these operands."""
    L = nat.lib()
    i64 = ctypes.c_int64
    dt, red = nat.dtype_code(x.dtype), nat.REDUCES['sum']
    m, e, (n, K) = rp.numel() - 1, c.numel(), x.shape
    dims = (i64(1), i64(m), i64(n), i64(K), i64(e))
    out = torch.empty(m, K, dtype=x.dtype, device=dev)
    ws = torch.full((L.tsamd_spmm_workspace_bytes(dt, red, *dims), ), SENTINEL, dtype=torch.uint8, device=dev)
    lay_rows, lay = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    per_id = L.tsamd_spmm_hot_rows_layout(dt, red, *dims, nat._ptr(x), nat._ptr(out), nat._ptr(ws), lay_rows)
    blocks = L.tsamd_spmm_hot_blocks_layout(dt, red, *dims, nat._ptr(x), nat._ptr(out), nat._ptr(ws), lay)
    return per_id, blocks, lay, ws, out, dims, dt, red


def _inspect(dev, rp, c, v, x):
    """tsamd_spmm (sum) on a sentinel-filled workspace of our own -> (out, flags [N] uint8, block words [WORDS] int64,
    the table's region as [WORDS * 64, row bytes] uint8)."""
    rp, c, x = rp.to(dev), c.to(dev), x.to(dev)
    v = None if v is None else v.to(dev)
    L = nat.lib()
    per_id, blocks, lay, ws, out, dims, dt, red = _hooks(dev, rp, c, x)
    assert blocks == 1 and per_id == 0, 'N >= 65536 takes the block route and only that'
    with torch.cuda.device(dev):
        st = L.tsamd_spmm(dt, red, nat._ptr(rp), nat._ptr(c), nat._ptr(v), nat._ptr(x), nat._ptr(out), nat._ptr(None),
                          *dims, nat._ptr(ws), ctypes.c_size_t(ws.numel()), nat.stream_ptr(dev))
    nat.check(st, 'tsamd_spmm')
    torch.cuda.synchronize()
    n, K = x.shape
    words = (n + 63) // 64
    row_bytes = K * x.element_size()
    flags = ws[lay[0]:lay[0] + n].clone()
    bw = ws[lay[1]:lay[1] + 4 * words].clone().view(torch.int32).to(torch.int64)
    assert (ws.data_ptr() + lay[2] - x.data_ptr()) == lay[3] * row_bytes, 'the table is a whole number of rows from mat'
    assert lay[2] + words * 64 * row_bytes <= ws.numel()
    table = ws[lay[2]:lay[2] + words * 64 * row_bytes].view(words * 64, row_bytes)
    return out, flags, bw, table


def _check_layout(dev, ops, rp, c, v, x):
    """The selected blocks are exactly those with at least kHotBlockMin flagged ids; their words hold rank + 1 in block
    order, the others 0; the table holds exactly the selected blocks' rows at the documented slots and the sentinel
    everywhere else (behind the last selected block, and where ids >= N of the partial block would sit); the result
    equals the op's bit for bit.  Returns (selected [WORDS] bool, flags)."""
    out, flags, bw, table = _inspect(dev, rp, c, v, x)
    n = x.shape[0]
    words = (n + 63) // 64
    assert bool(((flags == 0) | (flags == 1)).all())
    padded = torch.zeros(words * 64, dtype=torch.int64, device=dev)
    padded[:n] = flags
    sel = padded.view(words, 64).sum(1) >= _kmin()
    rank = torch.cumsum(sel.long(), 0) - sel.long()
    assert torch.equal(bw, torch.where(sel, rank + 1, torch.zeros_like(rank))), 'block words: rank + 1 of the selected blocks'
    ids = (sel.nonzero().flatten()[:, None] * 64 + torch.arange(64, device=dev)[None, :]).flatten()
    ids = ids[ids < n]
    r = rank[ids >> 6]
    rot = ((r * 0x9E3779B1) & 0xFFFFFFFF) >> 26
    slot = r * 64 + ((ids + rot) & 63)
    want = torch.full_like(table, SENTINEL)
    want[slot] = x.to(dev).contiguous().view(torch.uint8).view(n, -1)[ids]
    assert torch.equal(table, want), 'table: rows of the selected blocks at their slots, nothing else written'
    full = ops.torch_sparse.spmm_sum(None, rp.to(dev), c.to(dev), None if v is None else v.to(dev), None, None, x.to(dev))
    assert bits_equal(out, full)
    return sel, flags


@pytest.fixture(scope='module')
def common():
    return _rowptr(), _skewed(21), synth.values(E, seed=1) - 0.3, _features(N, 64, torch.float32)


@pytest.mark.parametrize('with_values', [True, False])
def test_common_shape(dev, ops, common, with_values):
    rp, c, v, x = common
    _both_ways(ops, dev, rp, c, v if with_values else None, x)


def test_layout(dev, ops, common):
    rp, c, v, x = common
    sel, _ = _check_layout(dev, ops, rp, c, v, x)
    S = int(sel.sum())
    print('selected %d of %d blocks' % (S, WORDS))
    assert 0 < S < WORDS, 'some blocks selected, some not'


def test_mixed_windows(dev, ops):
    """One block made hot by construction (64 ids x 30 k entries, spread over all rows) among blocks left cold, and a
    hub at id N - 1 in the partial block, which stays cold: hot and cold gathers meet in one window.  The entries the
    probe reads (every 128th) name the multiples of 8 of the hot block, so the probe fires."""
    hot_block = 517
    g = torch.Generator().manual_seed(31)
    col = torch.randint(0, N, (E, ), generator=g)
    pos = torch.randperm(E, generator=g)
    col[pos[:64 * 30000]] = hot_block * 64 + torch.arange(64).repeat(30000)
    col[pos[64 * 30000:64 * 30000 + 40000]] = N - 1
    col[::128] = hot_block * 64 + 8 * (torch.arange(E // 128) % 8)
    rp = _rowptr()
    v, x = synth.values(E, seed=2) - 0.3, _features(N, 64, torch.float32, seed=1)
    _both_ways(ops, dev, rp, col, v, x)
    sel, flags = _check_layout(dev, ops, rp, col, v, x)
    assert sel.nonzero().flatten().tolist() == [hot_block], 'the hot block and no other'
    assert int(flags[N - 1]) == 1 and not bool(sel[WORDS - 1]), 'the hub is flagged, its block is not selected'


def test_nothing_selected(dev, ops):
    """Skewed, and flagged ids spread at most 8 per block (fewer than the threshold): the sampled entries walk through
    multiples of 8.  The call succeeds, every block word is 0, not one byte of the table's region is written."""
    per_block = min(8, _kmin() - 1)
    g = torch.Generator().manual_seed(32)
    col = torch.randint(0, N, (E, ), generator=g)
    col[::3] &= ~7
    j = torch.arange(E // 32)
    col[::32] = ((j // per_block) % (WORDS - 1)) * 64 + 8 * (j % per_block)
    rp = _rowptr()
    v, x = synth.values(E, seed=3) - 0.3, _features(N, 64, torch.float32, seed=2)
    _both_ways(ops, dev, rp, col, v, x, reduces=('sum', ))
    sel, flags = _check_layout(dev, ops, rp, col, v, x)
    assert int(flags.sum()) > 0 and int(sel.sum()) == 0


def test_every_block_selected(dev, ops):
    """The sampled entries that the probe does not read walk through every id whose low six bits are below 40 (all 41
    ids of the partial block among them); the ones it reads are multiples of 8.  The table fills to its last block,
    whose rows of ids >= N stay untouched."""
    g = torch.Generator().manual_seed(33)
    col = torch.randint(0, N, (E, ), generator=g)
    col[::3] &= ~7
    ids = torch.arange(N)
    ids = ids[(ids & 63) < 40]
    j = torch.arange(E // 32)
    walk = ids[(j - j // 4 - 1).clamp(min=0) % ids.numel()]
    assert (E // 32) - (E // 128) >= ids.numel()
    col[::32] = torch.where(j % 4 == 0, 8 * ((j // 4) % (N // 8)), walk)
    rp = _rowptr()
    v, x = synth.values(E, seed=4) - 0.3, _features(N, 64, torch.float32, seed=3)
    _both_ways(ops, dev, rp, col, v, x, reduces=('sum', ))
    sel, _ = _check_layout(dev, ops, rp, col, v, x)
    assert int(sel.sum()) == WORDS


def test_uniform_graph_copies_nothing(dev, ops):
    """Uniform ids: the probe does not fire and every prologue kernel leaves at once.  The call is in scope (the layout
    exists), the flags were cleared and no id marked, no block word and not one byte of the table's region written."""
    g = torch.Generator().manual_seed(36)
    col = torch.randint(0, N, (E, ), generator=g)
    rp = _rowptr()
    v, x = synth.values(E, seed=6) - 0.3, _features(N, 64, torch.float32, seed=6)
    _both_ways(ops, dev, rp, col, v, x, reduces=('sum', ))
    out, flags, bw, table = _inspect(dev, rp, col, v, x)
    assert int(flags.sum()) == 0, 'an id was marked on a graph the probe does not flag'
    assert bool((bw == int.from_bytes(bytes([SENTINEL] * 4), 'little', signed=True)).all()), 'block words were written'
    assert bool((table == SENTINEL).all()), 'rows were copied'


def test_small_n_keeps_the_per_id_route(dev):
    n, m, e = 9001, 5000, 1300000
    g = torch.Generator().manual_seed(34)
    c = torch.randint(0, n, (e, ), generator=g)
    rp = torch.zeros(m + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(torch.randint(0, m, (e, ), generator=g), minlength=m), 0)
    x = _features(n, 64, torch.float32, seed=4)
    per_id, blocks = _hooks(dev, rp.to(dev), c.to(dev), x.to(dev))[:2]
    assert blocks == 0 and per_id == 1


@pytest.mark.parametrize('dtype', [torch.float64, torch.bfloat16])
def test_other_types_at_256_byte_rows(dev, ops, dtype):
    rp, c = _rowptr(), _skewed(35)
    K = 256 // torch.empty(0, dtype=dtype).element_size()
    v = (synth.values(E, seed=5) - 0.3).to(dtype)
    x = _features(N, K, dtype, seed=5)
    _both_ways(ops, dev, rp, c, v, x, reduces=('sum', ))
    sel, _ = _check_layout(dev, ops, rp, c, v, x)
    assert 0 < int(sel.sum()) < WORDS
