"""Every route of the SpMM forward's merge and fix-up kernels (csrc/spmm_kernels.h) against the fp64 oracle of
tests/spmm_forward_reference.py.  Every case goes through the C-ABI on a workspace of its own, filled with a sentinel
byte: the call's route (tsamd_spmm_route), the census of what it left there (partition table, tail_row, head_row) and
the expected values then come from one call.  A case asserts its route fields and census keys FIRST -- a case that no
longer reaches its target is a failure -- then compares in exact mode (small integers: every partial sum is exact in
any order, sums are compared bit for bit), then once with real values against the derived bound.  min / max and the
integer types are bit-exact, values and ids, always.  The device's partition table is held to the numpy partition in
every call."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import spmm_forward_reference as R

pytestmark = pytest.mark.gpu

F32, F64, F16, BF16, I32 = torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32
SENTINEL, GUARD = 0xAB, 64  # workspace fill; guard elements on either side of out / arg_out
MAXVEC = {F32: 4, F64: 2, F16: 4, BF16: 4, I32: 4}


def placed(t, off, dev, guard=True):
    """`t` on the device, `off` elements into a storage of its own with GUARD sentinel elements around it
    -> (view, whole buffer)"""
    g = GUARD if guard else 0
    buf = torch.empty(t.numel() + 2 * g + off, dtype=t.dtype, device=dev)
    buf.view(torch.uint8).fill_(0x5A)
    view = buf[g + off:g + off + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def guards_intact(view, buf, off):
    b = buf.view(torch.uint8)
    es, n = view.element_size(), view.numel()
    return bool((b[:(GUARD + off) * es] == 0x5A).all()) and bool((b[(GUARD + off + n) * es:] == 0x5A).all())


def call(dev, dtype, reduce, rowptr, col, value, x, arg32=False, offs=(0, 0, 0)):
    """One forward call -> dict(out, arg, route, table, tail_row, head_row, flag).  rowptr / col: numpy int64; value:
    fp64 numpy or None; x: fp64 numpy [N, K] or [B, N, K]; offs: elements that mat, out and arg_out sit into their
    storages."""
    minmax = reduce in ('min', 'max')
    xt = R.store(x, dtype) if dtype.is_floating_point else torch.from_numpy(x).to(dtype)
    vt = None if value is None else (R.store(value, dtype) if dtype.is_floating_point else torch.from_numpy(value).to(dtype))
    B = 1 if xt.dim() == 2 else xt.shape[0]
    N, K = xt.shape[-2:]
    M, E = len(rowptr) - 1, len(col)
    mat, _ = placed(xt, offs[0], dev, guard=False)
    out, out_buf = placed(torch.zeros(xt.shape[:-2] + (M, K), dtype=dtype), offs[1], dev)
    arg = arg_buf = None
    if minmax:
        arg, arg_buf = placed(torch.zeros(out.shape, dtype=torch.int32 if arg32 else torch.int64), offs[2], dev)
    rp, c = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
    v = None if vt is None else vt.to(dev)
    L, i64 = nat.lib(), ctypes.c_int64
    dt, red = nat.dtype_code(dtype), nat.REDUCES[reduce]
    dims = (i64(B), i64(M), i64(N), i64(K), i64(E))
    ws = torch.full((max(L.tsamd_spmm_workspace_bytes(dt, red, *dims), 256), ), SENTINEL, dtype=torch.uint8, device=dev)
    route = nat.spmm_route(dtype, reduce, B, M, N, K, E, mat=mat, out=out, arg_out=0 if arg is None else arg, arg32=arg32,
                           workspace=ws)
    assert route['workspace_bytes'] <= ws.numel()
    with torch.cuda.device(dev):
        head = (dt, red, nat._ptr(rp), nat._ptr(c), nat._ptr(v), nat._ptr(mat), nat._ptr(out), nat._ptr(arg), *dims,
                nat._ptr(ws), ctypes.c_size_t(ws.numel()))
        if arg32:
            st = L.tsamd_spmm_minmax_arg32(*head, None, ctypes.c_size_t(0), 0, nat.stream_ptr(dev))
        else:
            st = L.tsamd_spmm(*head, nat.stream_ptr(dev))
    nat.check(st, 'tsamd_spmm')
    torch.cuda.synchronize()
    assert guards_intact(out, out_buf, offs[1]), 'bytes written around out'
    assert arg is None or guards_intact(arg, arg_buf, offs[2]), 'bytes written around arg_out'
    P = route['P']
    words = lambda off, n: ws[off:off + 8 * n].view(torch.int64).cpu().numpy()  # noqa: E731
    res = {'out': out.cpu(), 'arg': None if arg is None else arg.cpu(), 'route': route,
           'table': words(route['table_off'], 2 * (P + 1)).reshape(P + 1, 2), 'tail_row': words(route['tail_row_off'], P),
           'head_row': words(route['head_row_off'], P),
           'flag': ws[route['relabel_flag_off']:route['relabel_flag_off'] + 16].view(torch.int32).cpu().numpy()}
    # the device's table is the numpy partition, with this call's snap
    assert np.array_equal(res['table'], R.partition(rowptr, route['items'], route['snap'])), 'partition table'
    return res


def census_of(res, rowptr):
    r = res['route']
    if r['P'] == 1:  # no fix-up launch: head_row of the only partition is whatever the merge kernel left (-1)
        return R.census(rowptr, res['table'], r['items'], r['snap'])
    return R.census(rowptr, res['table'], r['items'], r['snap'], res['tail_row'], res['head_row'])


def compare(res, rowptr, col, value, x, reduce, dtype, exact_mode, want=None):
    """exact mode: sums bit for bit, the mean inside the derived bound; real values: the derived bound; min / max: bits
    and ids."""
    exact, l1, arg = want if want is not None else R.oracle(rowptr, col, value, x, reduce, dtype)
    if reduce in ('min', 'max'):
        E = len(col)
        bad = R.minmax_mismatches(res['out'], res['arg'], exact, arg, dtype)
        assert bad == 0, '%d values / ids differ (%s %s)' % (bad, dtype, reduce)
        assert bool(((res['arg'] >= 0) & (res['arg'] <= E)).all())
        return
    if exact_mode and reduce == 'sum':
        bad = R.exact_mismatches(res['out'], exact, dtype)
        assert bad == 0, '%d sums differ in their bits (%s)' % (bad, dtype)
    bad, worst = R.real_violations(res['out'], exact, l1, rowptr, dtype, reduce)
    assert bad == 0, '%d elements outside the bound, worst error / bound %.3g (%s %s)' % (bad, worst, dtype, reduce)


def both_modes(dev, dtype, reduce, rowptr, N, K, B=None, seed=0, arg32=False, offs=(0, 0, 0), check=None):
    """exact mode, then real values once; `check(res)` asserts the case's route and census first."""
    assert R.exact_operands_ok(rowptr, dtype)
    col = R.columns(int(rowptr[-1]), N, seed)
    for exact_mode, operands in ((True, R.exact_operands), (False, R.real_operands)):
        v, x = operands(N, K, len(col), dtype, seed + 1, B=B)
        res = call(dev, dtype, reduce, rowptr, col, v, x, arg32=arg32, offs=offs)
        if check is not None:
            check(res)
        compare(res, rowptr, col, v, x, reduce, dtype, exact_mode)
    return res


def integer_case(dev, reduce, rowptr, N, K, offs, seed=0):
    col = R.columns(int(rowptr[-1]), N, seed)
    v, x = R.exact_operands(N, K, len(col), F32, seed + 1)
    res = call(dev, I32, reduce, rowptr, col, v, x, offs=offs)
    eo, ea = R.oracle_int(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(v).to(I32),
                          torch.from_numpy(x).to(I32), reduce, I32)
    assert torch.equal(res['out'], eo) and (ea is None or torch.equal(res['arg'], ea))
    return res


# ---- packet ladder ------------------------------------------------------------------------------------------------
SKEWED = R.build_skewed(1 << 10)[0]
LADDER_K = {F32: (64, 66, 65), BF16: (64, 66, 65), F16: (64, 66, 65), F64: (32, 33), I32: (64, 66, 65)}
PLACES = [('none', 0), ('mat', 1), ('mat', 2), ('out', 1), ('out', 2), ('arg', 1), ('arg', 2), ('all', 1), ('all', 2)]


def want_vec(dtype, K, reduce, arg32, offs):
    """packet_width by hand: the widest packet that divides K and every pointer's offset in bytes"""
    es = torch.empty(0, dtype=dtype).element_size()
    vec = MAXVEC[dtype]
    ids = 4 if arg32 else 8
    while vec > 1 and not (K % vec == 0 and (offs[0] * es) % (vec * es) == 0 and (offs[1] * es) % (vec * es) == 0 and
                           (reduce in ('sum', 'mean') or (offs[2] * ids) % (vec * ids) == 0)):
        vec //= 2
    return vec


def ladder_case(dev, dtype, K, where, off):
    offs = tuple(off if where in (name, 'all') else 0 for name in ('mat', 'out', 'arg'))
    seen = set()
    for reduce in R.REDUCES:
        for arg32 in ((False, True) if reduce in ('min', 'max') and dtype != I32 else (False, )):
            vec = want_vec(dtype, K, reduce, arg32, offs)

            def check(res):
                assert res['route']['vec'] == vec, (res['route'], vec)
                c = census_of(res, SKEWED)
                assert res['route']['fixup'] == 1 and c['cut_rows'] >= 10 and max(c['run_hist']) >= 3
            if dtype == I32:
                check(integer_case(dev, reduce, SKEWED, 500, K, offs))
            else:
                both_modes(dev, dtype, reduce, SKEWED, 500, K, arg32=arg32, offs=offs, check=check)
            seen.add(vec)
    return seen


@pytest.mark.parametrize('dtype', [F32, BF16, F64, F16, I32])
def test_packet_ladder_by_k(dev, dtype):
    widths = [v for K in LADDER_K[dtype] for v in ladder_case(dev, dtype, K, 'none', 0)]
    assert widths == ([4, 2, 1] if MAXVEC[dtype] == 4 else [2, 1])


@pytest.mark.parametrize('where,off', PLACES[1:])
@pytest.mark.parametrize('dtype', [F32, BF16, F64, F16, I32])
def test_packet_ladder_by_pointer(dev, dtype, where, off):
    """mat, out and arg_out (int64 and int32) one and two elements into their storage, each alone and all together;
    guard words around out and arg_out stay untouched (asserted in every call)."""
    seen = ladder_case(dev, dtype, LADDER_K[dtype][0], where, off)  # (every call asserts want_vec)
    if where == 'arg':
        assert MAXVEC[dtype] in seen  # sums ignore arg_out
        assert off == 2 or 1 in seen  # ids one element in: single elements, for int64 and for int32 ids
    elif off == 1:
        assert seen == {1}


# ---- lane groups --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [None, 3])
@pytest.mark.parametrize('slots', [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_lane_groups(dev, dtype, slots, B):
    """slots per row that are and are not a power of two (lanes with kok == false inside a group), one, two and three
    feature tiles (last tile one or two packets), each alone and with three batches on gridDim.y."""
    K = 4 * slots
    lpr = 1 << (min(slots, 64) - 1).bit_length()
    lgG = 6 - (lpr.bit_length() - 1)
    ktiles = -(-slots // 64)
    rowptr = R.build_skewed(300, seed=3, hub=400)[0]

    def check(res):
        r = res['route']
        assert (r['vec'], r['slots'], r['lpr'], r['lgG'], r['ktiles']) == (4, slots, lpr, lgG, ktiles), r
        assert r['family'].endswith('short' if lgG >= 3 else 'cooperative') and r['grid_y'] == (B or 1) * ktiles
        assert census_of(res, rowptr)['cut_rows'] >= 3
    for reduce in R.REDUCES:
        both_modes(dev, dtype, reduce, rowptr, 97, K, B=B, seed=slots, check=check,
                   arg32=reduce == 'min')  # (min with int32 ids, max with int64 ids)


# ---- fix-up chains --------------------------------------------------------------------------------------------------
CHAINS, CHAIN_KEYS = R.build_chains(128)
RUNS = {1, 2, 7, 8, 9, 16, 63, 64, 65, 128, 199}


@pytest.mark.parametrize('K,B', [(8, None), (64, None), (132, None), (260, None), (8, 2), (260, 2)])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_fixup_chains(dev, dtype, K, B):
    """Cut rows with 1, 2, 7, 8, 9, 16, 63, 64, 65, 128 and 199 tail records in front of their head: every branch of
    spmm_fixup_kernel by chain length, at K = 8 (short-row merge kernel), 64, 132 and 260 (the second fetch round of
    the fix-up, two feature tiles); K = 8 and 260 again with a grid row per batch."""
    def check(res):
        r = res['route']
        assert r['items'] == 128 and r['fixup'] == 1 and r['family'] == ('short' if K == 8 else 'cooperative')
        c = census_of(res, CHAINS)
        if r['snap'] == 0:
            assert RUNS <= set(c['run_hist']), sorted(c['run_hist'])
            for k in ('empty_head', 'cut_last_row', 'inside_one_row', 'boundary_on_row_start', 'incoming_row_ends'):
                assert c[k] >= CHAIN_KEYS[k], k
        else:  # min / max: the snap keeps short rows whole, the chains stay
            assert RUNS <= set(c['run_hist']) and c['cut_last_row'] == 1 and c['snapped'] >= 1
    for reduce in R.REDUCES:
        both_modes(dev, dtype, reduce, CHAINS, 64, K, B=B, seed=K, check=check)


@pytest.mark.parametrize('dtype', [F32, BF16])
def test_one_row_one_partition_two_partitions(dev, dtype):
    one = R.build_one_row(128)[0]

    def check_one(res):
        c = census_of(res, one)
        assert c['run_hist'] == {3: 1} and c['cut_last_row'] == 1 and res['route']['P'] == 4
    for reduce in R.REDUCES:
        both_modes(dev, dtype, reduce, one, 64, 64, check=check_one)
        for P in (1, 2):
            rowptr = R.build_partitions(128, P)[0]

            def check(res):
                assert res['route']['P'] == P and res['route']['fixup'] == P - 1
            both_modes(dev, dtype, reduce, rowptr, 64, 64, check=check)


# ---- ties and winners across pieces ---------------------------------------------------------------------------------
def tie_operands(rowptr, named, K, B, variant, seed=5):
    """N = 17 rows of X: 0..9 random small integers, 10 the long row's filler, 11..13 its per-feature winners, 14 NaN,
    15 / 16 = -0.0 / +0.0"""
    rng = np.random.default_rng(seed)
    E = int(rowptr[-1])
    col = rng.integers(0, 10, E).astype(np.int64)
    x = np.zeros((17, K))
    x[:10] = rng.integers(-3, 4, (10, K))
    x[10] = 3.0
    x[11:14] = 2.0
    for t in range(3):
        x[11 + t, t::3] = 5.0  # feature k is won by special column 11 + k % 3
    x[14] = np.nan
    x[15], x[16] = -0.0, 0.0
    s, e = rowptr[named['long']], rowptr[named['long'] + 1]
    col[s:e] = 10
    spots = None
    if variant == 'unique':
        spots = np.array([s + 5, s + (e - s) // 2 + 3, e - 2])  # the first, a middle and the last piece
        col[spots] = [11, 12, 13]
    s, e = rowptr[named['nan']], rowptr[named['nan'] + 1]
    col[s:e] = 14
    s, e = rowptr[named['zeros']], rowptr[named['zeros'] + 1]
    col[s:e] = np.where(np.arange(e - s) % 2 == 0, 15, 16)
    if B is not None:
        x = np.stack([x, np.roll(x, 1, axis=-1)])
        x[1, 14] = np.nan
    return col, x, spots


@pytest.mark.parametrize('arg32', [False, True])
@pytest.mark.parametrize('B', [None, 2])
@pytest.mark.parametrize('K', [8, 64, 260])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_ties_and_winners_across_pieces(dev, dtype, K, B, arg32):
    """The fix-up's tie rule (v == val && a < arg, folded from the last piece backwards) where it decides: a 70-piece
    row of equal entries; unique winners in the first, a middle and the last piece (a different one per feature inside
    one packet); a cut row of NaN; a cut row of -0.0 / +0.0; rows of `snap` and snap + 1 entries across a diagonal."""
    probe = nat.spmm_route(dtype, 'max', B or 1, 400, 17, K, 10000, arg32=arg32)
    rowptr, _, named = R.build_ties(probe['items'], probe['snap'])
    E = int(rowptr[-1])
    first = {k: int(rowptr[r]) for k, r in named.items()}
    for variant in ('equal', 'unique'):
        col, x, spots = tie_operands(rowptr, named, K, B, variant)
        for reduce in ('max', 'min'):
            xs = x if reduce == 'max' else -x
            res = call(dev, dtype, reduce, rowptr, col, None, xs, arg32=arg32)
            r = res['route']
            assert (r['items'], r['snap']) == (probe['items'], probe['snap']) and r['snap'] > 0
            assert r['family'] == ('arg32_' if arg32 else '') + ('short' if K == 8 else 'cooperative')
            c = census_of(res, rowptr)
            assert c['runs'][named['long']] == 69 and named['nan'] in c['runs'] and named['zeros'] in c['runs']
            assert named['snap'] not in c['runs'] and c['runs'].get(named['snap1']) == 1 and c['snapped'] >= 1
            compare(res, rowptr, col, None, xs, reduce, dtype, True)
            out, arg = res['out'].reshape(-1, len(rowptr) - 1, K), res['arg'].reshape(-1, len(rowptr) - 1, K)
            sign = 1.0 if reduce == 'max' else -1.0
            for b in range(out.shape[0]):
                if variant == 'equal':
                    assert bool((arg[b, named['long']] == first['long']).all()), 'id 0 of the row wins every feature'
                else:
                    k = (np.arange(K) - b) % K  # batch 1 holds the features rolled by one
                    assert np.array_equal(arg[b, named['long']].numpy(), spots[k % 3])
                    assert bool((out[b, named['long']].double() == sign * 5.0).all())
                assert bool((arg[b, named['nan']] == E).all()), 'a row of NaN has no winner'
                assert bool((out[b, named['nan']].double().abs() == R.INIT[dtype]).all())
                assert bool((arg[b, named['zeros']] == first['zeros']).all()), 'the first zero wins'
                zero_bits = R.bits_of(out[b, named['zeros']])
                assert bool((zero_bits == R.bits_of(R.store(np.array([-0.0 * sign]), dtype))).all())


# ---- short-row batches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reduce', ['sum', 'max'])
@pytest.mark.parametrize('slots', [1, 2, 4, 8])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_short_row_batches(dev, dtype, slots, reduce):
    """short_rows' decisions, each counted from the device's table: rows of exactly 8 lpr and 8 lpr + 1 entries as
    member 0, 1 and a middle one; runs of 1, 2, G and G + 1 short rows; 200 empty rows (the row-end reload); a cut
    row's end followed by a batch; an unfinished short last row; navail < 2."""
    K = 4 * slots
    probe = nat.spmm_route(dtype, reduce, 1, 1000, 64, K, 5000)
    rowptr, keys = R.build_short(probe['items'], probe['lgG'])

    def check(res):
        r = res['route']
        assert (r['family'], r['lgG'], r['items'], r['lpr']) == ('short', probe['lgG'], probe['items'], slots)
        c = R.short_census(rowptr, res['table'], r['lgG'])
        if reduce == 'sum':
            for k in keys:
                assert c[k] >= 1, (k, c)
            assert c['longest_batch'] == 1 << r['lgG'] and {2, 1 << r['lgG']} <= set(c['batch_sizes'])
        else:  # the snap moves boundaries: what must still be there
            for k in ('batches', 'reloads', 'limit_row_member_1', 'over_limit_member_1', 'ended_by_long_2plus'):
                assert c[k] >= 1, (k, c)
        census_of(res, rowptr)
    both_modes(dev, dtype, reduce, rowptr, 64, K, seed=slots, check=check)


# ---- partition length -------------------------------------------------------------------------------------------------
LENGTHS = R.LENGTH_CASES  # (dtype, K, M + E, items)


@pytest.mark.parametrize('dtype,K,total,items', LENGTHS)
def test_partition_length(dev, dtype, K, total, items):
    """items above the 128 every small graph runs: 4096 rows of skewed lengths over 64 columns, the linear oracle.
    sum in exact mode; min / max without values (their snap is 128 from items = 256 on)."""
    M, N = 4096, 64
    rowptr = R.build_total(M, total)
    assert R.exact_operands_ok(rowptr, dtype)
    col = R.columns(int(rowptr[-1]), N, 1)
    _, x = R.exact_operands(N, K, 1, dtype, 2)
    res = call(dev, dtype, 'sum', rowptr, col, None, x)
    assert res['route']['items'] == items and res['route']['P'] == -(-total // items)
    c = census_of(res, rowptr)
    assert c['cut_rows'] >= 100 and max(c['run_hist']) >= 64 and c['inside_one_row'] >= 64
    exact, l1 = R.linear_oracle(rowptr, col, None, x, 'sum', N)
    compare(res, rowptr, col, None, x, 'sum', dtype, True, want=(exact, l1, None))
    for reduce in ('max', 'min'):
        res = call(dev, dtype, reduce, rowptr, col, None, x)
        assert res['route']['items'] == items and res['route']['snap'] == min(128, items // 2)
        assert census_of(res, rowptr)['snapped'] >= 1
        exact, arg = R.linear_minmax(rowptr, col, x, reduce, N, dtype)
        compare(res, rowptr, col, None, x, reduce, dtype, True, want=(exact, None, arg))


# ---- full relabelled copy ---------------------------------------------------------------------------------------------
def full_copy_graph(skewed):
    n, m, e = 4096, 2048, 1 << 20
    rng = np.random.default_rng(21)
    col = rng.integers(0, n, e).astype(np.int64)
    if skewed:
        col[::3] &= ~7  # low-bit skew, as the probe looks for
    lens = rng.multinomial(e, np.ones(m) / m)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col, n


@pytest.mark.parametrize('skewed', [True, False])
@pytest.mark.parametrize('dtype,reduce,K,B,mat_off', [(F32, 'sum', 64, 2, 0), (F32, 'max', 64, None, 0),
                                                      (F64, 'max', 32, None, 0), (F32, 'sum', 64, None, 2)])
def test_full_copy(dev, dtype, reduce, K, B, mat_off, skewed):
    """relabel_mode 2 outside the hot scope: two batches, fp32 / fp64 max, a mat 8 bytes into its storage -- the
    smallest shape relabel_possible admits, on a `col` the probe flags and on one it does not (read from the call's
    probe counters)."""
    rowptr, col, n = full_copy_graph(skewed)
    v, x = R.exact_operands(n, K, len(col), dtype, 22, B=B)
    res = call(dev, dtype, reduce, rowptr, col, v, x, offs=(mat_off, 0, 0))
    r, f = res['route'], res['flag']
    assert (r['relabel'], r['copy'], r['family']) == (2, 1, 'cooperative'), r
    assert r['vec'] == (2 if mat_off else MAXVEC[dtype])
    flagged = f[3] >= 4096 and (f[1] * 4 > f[3] or f[2] * 16 > f[3])
    assert f[3] == 64 * 256 and flagged == skewed, f
    census_of(res, rowptr)
    compare(res, rowptr, col, v, x, reduce, dtype, True)


# ---- through the operators --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [8, 64, 260])
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_chains_through_ops_and_matmul(dev, dtype, K):
    """The chain graph again through torch.ops.torch_sparse.spmm_* and SparseTensor.matmul, where the pointers cannot be
    chosen: the same exact comparison."""
    import pytorch_sparse_amd as ts
    col = R.columns(int(CHAINS[-1]), 64, 3)
    v, x = R.exact_operands(64, K, len(col), dtype, 4)
    rp, c = torch.from_numpy(CHAINS).to(dev), torch.from_numpy(col).to(dev)
    vt, xt = R.store(v, dtype).to(dev), R.store(x, dtype).to(dev)
    A = ts.SparseTensor(rowptr=rp, col=c, value=vt, sparse_sizes=(len(CHAINS) - 1, 64), is_sorted=True, trust_data=True)
    ops = torch.ops.torch_sparse
    for reduce in R.REDUCES:
        want = R.oracle(CHAINS, col, v, x, reduce, dtype)
        if reduce == 'sum':
            got = (ops.spmm_sum(None, rp, c, vt, None, None, xt), None)
        elif reduce == 'mean':
            got = (ops.spmm_mean(None, rp, c, vt, None, None, None, xt), None)
        else:
            got = getattr(ops, 'spmm_' + reduce)(rp, c, vt, xt)
        compare({'out': got[0].cpu(), 'arg': None if got[1] is None else got[1].cpu()}, CHAINS, col, v, x, reduce, dtype,
                True, want=want)
        o = A.matmul(xt, reduce=reduce)
        if reduce in ('min', 'max'):
            assert R.bits_of(o).equal(R.bits_of(R.store(want[0], dtype)))
        else:
            compare({'out': o.cpu(), 'arg': None}, CHAINS, col, v, x, reduce, dtype, True, want=want)
