"""Every route of the min / max backward against tests/minmax_bw_reference.py: the winners come from the forward's
oracle on the host (never from the device), the records are compared word for word with the layout restated there, the
gradients bit for bit on small integers and within the derived bounds on real values.  Every output lies between guard
words in a buffer filled with bytes of 85; which route a case takes is asserted through tsamd_spmm_minmax_bw_route
(and tsamd_spmm_route for the forward) before anything is compared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import minmax_bw_reference as mr
from tests import spmm_forward_reference as fr

pytestmark = pytest.mark.gpu
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
GUARD = 64   # elements in front of and behind every output that no call may touch
FILL = 85


# ---- guarded outputs ---------------------------------------------------------------------------------------------
class Guarded:
    """`numel` elements of `dtype` inside a buffer of bytes of 85, `skew` bytes off the 16-byte boundary"""

    def __init__(self, numel, dtype, dev, skew=0):
        es = torch.empty(0, dtype=dtype).element_size()
        assert skew % es == 0
        self.pad = GUARD * es + skew
        self.nbytes = numel * es
        self.raw = torch.full((self.nbytes + 2 * GUARD * es + 16, ), FILL, dtype=torch.uint8, device=dev)
        self.out = self.raw[self.pad:self.pad + self.nbytes].view(dtype)
        assert self.out.data_ptr() % 16 == skew % 16

    def intact(self):
        return bool((self.raw[:self.pad] == FILL).all()) and bool((self.raw[self.pad + self.nbytes:] == FILL).all())


def _d(a, dev, dtype=None):
    if a is None:
        return None
    if dtype is not None:
        return fr.store(a, dtype).to(dev)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Dev:
    """a case's operands on the device"""

    def __init__(self, c, dev):
        self.c, self.dev = c, dev
        self.rowptr, self.col, self.row = _d(c.rowptr, dev), _d(c.col, dev), _d(c.row, dev)
        colptr, perm = c.csc()
        self.colptr, self.perm = _d(colptr, dev), _d(perm, dev)
        self.value, self.x, self.g = _d(c.value, dev, c.dtype), _d(c.x, dev, c.dtype), _d(c.gout, dev, c.dtype)
        self.arg64 = _d(np.asarray(c.arg, np.int64), dev)
        self.arg32 = self.arg64.to(torch.int32)

    def outputs(self, want_value, want_mat=True, skew=0):
        c = self.c
        gv = Guarded(c.E, c.dtype, self.dev) if want_value else None
        gm = Guarded(c.B * c.N * c.K, c.dtype, self.dev, skew) if want_mat else None
        return gv, gm

    def route(self, winners, want_value, want_mat=True, gm=None, x=None, g=None):
        c = self.c
        return nat.spmm_minmax_bw_route(winners, c.dtype, c.B, c.M, c.N, c.K, c.E, want_value, want_mat,
                                        mat=self.x if x is None else x, grad_out=self.g if g is None else g,
                                        grad_mat=0 if gm is None else gm.out)

    def run(self, winners, want_value, want_mat=True, skew=0, rec=None, x=None, g=None):
        """one C-ABI call into guarded outputs -> (gv, gm) tensors or None; asserts the guards"""
        gv, gm = self.outputs(want_value, want_mat, skew)
        x, g = self.x if x is None else x, self.g if g is None else g
        o = dict(gv=None if gv is None else gv.out, gm=None if gm is None else gm.out)
        csr, csc = (self.rowptr, self.col), (self.colptr, self.perm, self.row)
        if winners == 'none':
            nat.spmm_minmax_bw(*csr, self.value, x, g, self.arg64, want_value, want_mat, **o)
        elif winners == 'records':
            nat.spmm_minmax_bw_csc_records(*csr, self.c.has_value, x, g, rec, *csc, want_value=want_value, **o)
        else:
            nat.spmm_minmax_bw_csc(*csr, self.value, x, g, self.arg64 if winners == 'ids64' else self.arg32, *csc,
                                   want_value=want_value, want_mat=want_mat, **o)
        torch.cuda.synchronize()
        assert (gv is None or gv.intact()) and (gm is None or gm.intact()), 'a guard word was written'
        shape = np.shape(self.c.x)
        return (None if gv is None else gv.out.clone()), (None if gm is None else gm.out.clone().view(shape))


def _check(c, gv, gm, exact, mat_bound, tag):
    """grad_value / grad_mat (None: not asked for) against the reference, in the case's mode.  Every figure is printed
    before it is asserted."""
    ref = c.ref
    if exact:
        mr.assert_exact_mode(ref, c.dtype)
        bad_m = None if gm is None else mr.exact_mismatches(gm, ref['gm'], c.dtype)
        bad_v = None if gv is None else mr.exact_mismatches(gv, ref['gv'], c.dtype)
        print(tag, 'exact: mismatching grad_mat', bad_m, 'grad_value', bad_v)
        assert not bad_m and not bad_v, (tag, bad_m, bad_v)
        return
    if gm is not None:
        bound = {'scatter': lambda: mr.bound_scatter_mat(ref['gm_l1'], ref['gm_n'], c.dtype),
                 'pull': lambda: mr.bound_pull_mat(ref['gm'], ref['gm_l1'], ref['gm_n'], c.dtype),
                 'shadow': lambda: mr.bound_shadow_mat(ref['gm'], ref['gm_l1'], ref['gm_n'], c.dtype)}[mat_bound]()
        bad, ratio = mr.violations(gm, ref['gm'], bound, c.dtype)
        print(tag, 'grad_mat (%s bound): outside' % mat_bound, bad, 'worst ratio', ratio)
        assert bad == 0, (tag, 'grad_mat', bad, ratio)
    if gv is not None:
        bad, ratio = mr.violations(gv, ref['gv'], mr.bound_value(ref['gv'], ref['gv_l1'], c.dtype, c.B * c.K), c.dtype)
        print(tag, 'grad_value: outside', bad, 'worst ratio', ratio)
        assert bad == 0, (tag, 'grad_value', bad, ratio)


def _same_bits(a, b):
    return (a is None and b is None) or bool((fr.bits_of(a) == fr.bits_of(b)).all())


def _records_on_device(c, dev):
    """the REFERENCE's records, for the entries that read records"""
    rec = torch.zeros(_nrec(c), dtype=torch.int32, device=dev)
    flat = torch.from_numpy(c.rec.reshape(-1).view(np.int32).copy())
    rec[:flat.numel()] = flat.to(dev)
    return rec


def _nrec(c):
    return nat.lib().tsamd_spmm_minmax_records_bytes(nat._i64(c.B), nat._i64(c.K), nat._i64(c.E)) // 4


def _written_records(c, buf):
    """the [B, E, S] words a writer left in a guarded buffer"""
    S = mr.record_words(c.K)[1]
    assert buf.intact(), 'a guard word of the records was written'
    return buf.out[:c.B * c.E * S].cpu().numpy().view(np.uint32).reshape(c.B, c.E, S)


def _winrec(d):
    c = d.c
    buf = Guarded(_nrec(c), torch.int32, d.dev)
    nat.spmm_minmax_winrec(d.row, d.value, d.arg32, c.K, rec=buf.out, dtype=c.dtype)
    torch.cuda.synchronize()
    return _written_records(c, buf)


def _forward_records(d):
    """tsamd_spmm_minmax_records into guarded `out` and records -> (mismatching out elements, record words)"""
    c = d.c
    out = Guarded(c.B * c.M * c.K, c.dtype, d.dev)
    buf = Guarded(_nrec(c), torch.int32, d.dev)
    nat.spmm_minmax_records(d.rowptr, d.col, d.value, d.x, c.reduce, d.row, out=out.out, rec=buf.out)
    torch.cuda.synchronize()
    assert out.intact()
    want = fr.store(c.forward[0], c.dtype)
    bad = int((fr.bits_of(out.out) != fr.bits_of(want.reshape(-1))).sum())
    return bad, _written_records(c, buf)


# ---- records, word for word --------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', mr.W_LADDER)
def test_records_at_every_width(dev, K):
    """minmax_winrec_kernel (int32 ids directly, int64 ids through the first step of tsamd_spmm_minmax_bw_csc, observed
    in its gradients) and tsamd_spmm_minmax_records on the tiny graph, at every record width W of the ladder: W = 1, 5,
    9 and 33 have no bitmap word, W = 4 takes the whole-chunk store for its full chunks and the other path for the last,
    W = 32 is the last width whose bitmap is read, W = 34 has a bitmap word that must be ignored (one entry's only winner
    sits in feature K - 1 >= 1024).  Then the three pulls read what was written -- the records entry reads the
    REFERENCE's records -- and must give the reference's gradients, twice the same bits."""
    W, S = mr.record_words(K)
    for dtype, reduce, has_value, B, exact in ((F32, 'max', True, None, True), (BF16, 'min', False, None, False),
                                               (F64, 'max', True, 2, False), (F16, 'min', True, None, False)):
        c = mr.tiny_case(K, dtype, reduce, has_value, exact, seed=K, B=B, plant_high=K > 1024)
        d = Dev(c, dev)
        tag = ('K', K, str(dtype), reduce, has_value, B)
        r = d.route('ids32', False)
        assert (r['status'], r['mat'], r['write_records'], r['W'], r['S'], r['has_z']) == \
            (0, 'pull', 1, W, S, int(mr.masked_has_z(K))), tag
        fw = nat.spmm_route(dtype, reduce, c.B, c.M, c.N, K, c.E, mat=d.x, arg32=True)
        bad = mr.record_mismatches(_winrec(d), c.rec, K)
        print(tag, 'winrec: mismatching words', bad)
        assert bad == 0, tag
        bad_out, words = _forward_records(d)
        bad = mr.record_mismatches(words, c.rec, K)
        print(tag, 'forward (records instantiation %d): out' % fw['records'], bad_out, 'words', bad)
        assert bad_out == 0 and bad == 0, tag
        es = mr.element_size(dtype)
        sddmm = has_value and (K * es) % 16 == 0
        for winners in ('ids64', 'ids32', 'records'):
            want_value = sddmm or (has_value and winners == 'ids64')
            r = d.route(winners, want_value)
            assert r['status'] == 0 and r['mat'] == 'pull' and r['write_records'] == (winners != 'records'), (tag, winners)
            assert r['value'] == ('none' if not want_value else ('masked_sddmm' if sddmm else 'row_parallel')), (tag, winners)
            rec = _records_on_device(c, dev) if winners == 'records' else None
            gv, gm = d.run(winners, want_value, rec=rec)
            _check(c, gv, gm, exact, 'pull', tag + (winners, ))
            gv2, gm2 = d.run(winners, want_value, rec=rec)
            assert _same_bits(gv, gv2) and _same_bits(gm, gm2), (tag, winners, 'two runs differ')


FORWARD_CASES = [(128, BF16, 1, None, False), (100, F16, 1, None, False), (64, BF16, 2, None, True),
                 (256, F32, 2, None, True), (132, BF16, 2, None, False), (64, F32, 0, None, True),
                 (128, BF16, 1, 2, False), (64, F16, 2, 2, False)]


@functools.lru_cache(maxsize=None)
def _forward_case(K, dtype, B, exact):
    route = nat.spmm_route(dtype, 'max', B or 1, 100, 30002, K, 30000, arg32=True)
    long_rows, winners = ((1025, ), ('one', 64, 65)) if B else ((1025, 3001), mr.LONG_WINNERS)
    return mr.build_record_forward(K, route, dtype, 'max', True, exact, seed=3, B=B, long_rows=long_rows,
                                   long_winners=winners), route


@pytest.mark.parametrize('K,dtype,records,B,exact', FORWARD_CASES)
def test_record_writing_forward_at_its_thresholds(dev, K, dtype, records, B, exact):
    """tsamd_spmm_minmax_records in both instantiations (records 1: 97..128 features, 2: the others; 0: fp32 K = 64 keeps
    ids and the entry makes the records from them) on rows of snap / snap + 1 entries across a partition boundary, cut
    rows of 129 .. 1024 entries (the whole-row rewrite) and of 1025 / 3001 entries with 0, 1, 63, 64, 65 and K distinct
    winners (blank pieces and the distinct-winner walk), also with B = 2.  `out` bit for bit, every defined word of
    every record; then the records route on what the forward wrote."""
    c, route = _forward_case(K, dtype, B, exact)
    d = Dev(c, dev)
    fw = nat.spmm_route(dtype, 'max', c.B, c.M, c.N, K, c.E, mat=d.x, arg32=True)
    assert fw['records'] == records and (fw['items'], fw['snap']) == (route['items'], route['snap']) and fw['fixup'] == 1
    bad_out, words = _forward_records(d)
    bad = mr.record_mismatches(words, c.rec, K)
    print('forward K', K, dtype, 'B', B, ': out', bad_out, 'record words', bad)
    assert bad_out == 0 and bad == 0
    bad = mr.record_mismatches(_winrec(d), c.rec, K)
    assert bad == 0, ('winrec', bad)
    rec = torch.from_numpy(np.ascontiguousarray(words).view(np.int32).reshape(-1)).to(dev)
    full = torch.zeros(_nrec(c), dtype=torch.int32, device=dev)
    full[:rec.numel()] = rec
    want_value = (K * mr.element_size(dtype)) % 16 == 0
    r = d.route('records', want_value)
    assert (r['status'], r['mat'], r['write_records']) == (0, 'pull', 0)
    assert r['value'] == ('masked_sddmm' if want_value else 'none')
    gv, gm = d.run('records', want_value, rec=full)
    _check(c, gv, gm, exact, 'pull', ('records route K', K, str(dtype), B))


# ---- the scatter / row-parallel kernel ----------------------------------------------------------------------------
SCATTER_K = (64, 32, 16, 8, 4, 2, 1, 65, 127, 129)


@functools.lru_cache(maxsize=None)
def _row_parallel(K, dtype, exact, reduce):
    route = nat.spmm_minmax_bw_route('none', dtype, 1, 100, 100, K, 1000, True, True)
    return mr.build_row_parallel(K, route, dtype, reduce, True, exact, seed=K)


@pytest.mark.parametrize('dtype,exact,reduce', [(BF16, True, 'max'), (F16, False, 'min'), (F32, True, 'min'),
                                                (F64, False, 'max'), (BF16, False, 'max')])
@pytest.mark.parametrize('K', SCATTER_K)
def test_scatter_and_row_parallel_at_the_lds_capacity(dev, K, dtype, exact, reduce):
    """spmm_minmax_bw_kernel<.., GMAT, GVAL> in its three forms, for every lane-group width (K = 64 .. 1) and the tile
    loop (65, 127, 129): rows of cap - 1 .. 2 cap + 1 entries with winners at positions cap - 1 and cap, three passes
    next to one in a wave, a hub column, packed pairs that share a winner / differ / have one winner.  The same kernel
    behind tsamd_spmm_minmax_bw_csc (int64 ids) where rows are no 16-byte packets; the masked SDDMM where they are."""
    c = _row_parallel(K, dtype, exact, reduce)
    d = Dev(c, dev)
    narrow = dtype in (BF16, F16)
    tag = ('K', K, str(dtype), 'exact' if exact else 'real')
    for want_value, want_mat in ((True, True), (False, True), (True, False)):
        gvb, gmb = d.outputs(want_value, want_mat)
        r = d.route('none', want_value, want_mat, gm=gmb)
        odd = (c.B * c.N * K) % 2 == 1
        assert (r['status'], r['lgG'], r['cap']) == (0, mr.scatter_lgG(K), 256 >> mr.scatter_lgG(K)), tag
        assert r['value'] == ('row_parallel' if want_value else 'none') and r['mat'] == ('scatter' if want_mat else 'none')
        if want_mat:
            assert r['shadow'] == int(narrow and odd), tag
            assert r['packed'] == ('plain' if not narrow or odd else ('merge_pairs' if K % 2 == 0 else 'idx_parity')), tag
        gv, gm = d.run('none', want_value, want_mat)
        bound = 'shadow' if (want_mat and r['shadow']) else 'scatter'
        _check(c, gv, gm, exact, bound, tag + (want_value, want_mat, r['packed'], r['shadow']))
    # the pull on int64 ids: grad_value by the row-parallel kernel or by the masked SDDMM
    sddmm = (K * mr.element_size(dtype)) % 16 == 0
    r = d.route('ids64', True)
    assert (r['status'], r['mat'], r['value']) == (0, 'pull', 'masked_sddmm' if sddmm else 'row_parallel'), tag
    # the masked sum has no side-by-side kernel: cooperative also where a plain sum would go short (8 packets and fewer:
    # K <= 32 fp32, <= 16 fp64, <= 32 of the 2-byte types)
    assert r['family'] == 'cooperative' and (r['sum_lgG'] >= 3) == (-(-K // r['vec']) <= 8), tag
    assert r['sum_lgG'] >= 3 or K > 16, tag
    gv, gm = d.run('ids64', True)
    _check(c, gv, gm, exact, 'pull', tag + ('ids64 pull', r['value']))
    gv2, gm2 = d.run('ids64', True)
    assert _same_bits(gv, gv2) and _same_bits(gm, gm2), (tag, 'two runs differ')
    r = d.route('ids64', True, False)  # grad_value alone: the row-parallel kernel whatever the row size
    assert (r['status'], r['mat'], r['value']) == (0, 'none', 'row_parallel'), tag
    gv, _ = d.run('ids64', True, False)
    _check(c, gv, None, exact, 'pull', tag + ('ids64, grad_value alone', ))


@pytest.mark.parametrize('dtype', [BF16, F16])
@pytest.mark.parametrize('exact', [True, False], ids=['exact', 'real'])
def test_fp32_shadow_of_the_packed_scatter(dev, dtype, exact):
    """f16 / bf16 grad_mat through the fp32 shadow and narrow_from_f32_kernel: an odd element count (N = 5, K = 3) and an
    even one whose buffer starts 2 bytes into a 4-byte word."""
    for N, K, skew in ((5, 3, 0), (5, 4, 2), (6, 3, 2)):
        c = mr.build_small(N, K, 40, dtype, 'max', True, exact, seed=N * K + skew, deg=5)
        d = Dev(c, dev)
        _, gmb = d.outputs(False, True, skew)
        r = d.route('none', True, True, gm=gmb)
        assert (r['status'], r['shadow'], r['packed'], r['mat']) == (0, 1, 'plain', 'scatter')
        assert r['shadow_bytes'] == 256 == -(-4 * N * K // 256) * 256
        for want_value in (True, False):
            gv, gm = d.run('none', want_value, True, skew=skew)
            _check(c, gv, gm, exact, 'shadow', ('shadow', N, K, skew, str(dtype), want_value))
        # next to it: the same operands on an aligned buffer of even count take the packed atomics
        if skew:
            r = d.route('none', True, True)
            assert r['shadow'] == 0 and r['packed'] == ('merge_pairs' if K % 2 == 0 else 'idx_parity')
            gv, gm = d.run('none', True, True)
            _check(c, gv, gm, exact, 'scatter', ('packed', N, K, str(dtype)))


# ---- the masked sum and the masked SDDMM -------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,exact,has_value,B', [(F32, True, True, None), (BF16, False, True, None),
                                                     (F16, False, False, None), (F64, False, True, None),
                                                     (F32, True, True, 2)])
def test_masked_sum_over_cut_hub_columns(dev, dtype, exact, has_value, B):
    """The pull's masked sum on a transposed pattern of build_chains: hub columns cut into 2 .. 200 pieces (every chain
    length the fix-up branches on), columns with no entry (written as zeros), a column whose entries all lose, a cut
    last column -- records (the reference's), int32 and int64 ids, with the masked SDDMM."""
    K = 128 if B is None else 32
    probe = nat.spmm_minmax_bw_route('records', dtype, B or 1, 3000, 600, K, 60000)
    c = mr.build_masked_sum(probe['items'], K, dtype, 'max', has_value, exact, seed=2, B=B,
                            max_len=None if B is None else 9 * probe['items'])
    d = Dev(c, dev)
    for winners in ('records', 'ids32', 'ids64'):
        r = d.route(winners, has_value)
        assert (r['status'], r['mat'], r['items'], r['fixup']) == (0, 'pull', probe['items'], 1), winners
        assert r['value'] == ('masked_sddmm' if has_value else 'none') and r['P'] > 200 * (B is None)
        assert r['sddmm'] == ('pipelined' if has_value else 'none')
        rec = _records_on_device(c, dev) if winners == 'records' else None
        gv, gm = d.run(winners, has_value, rec=rec)
        tag = ('masked sum', str(dtype), winners, B)
        _check(c, gv, gm, exact, 'pull', tag)
        gv2, gm2 = d.run(winners, has_value, rec=rec)
        assert _same_bits(gv, gv2) and _same_bits(gm, gm2), (tag, 'two runs differ')
    empty = np.diff(c.csc()[0]) == 0
    assert empty.any() and bool((gm.cpu().reshape(c.B, c.N, K)[:, empty] == 0).all())


@pytest.mark.parametrize('dtype', [BF16, F16, F32, F64])
@pytest.mark.parametrize('packets', [1, 2, 3, 4, 8, 16, 24, 32, 64, 65])
def test_masked_sddmm_at_every_packet_count(dev, dtype, packets):
    """grad_value from records: spmm_value_bw_masked_kernel for 1 .. 64 packets per row (every lane-group width, a count
    that is no power of two), spmm_value_bw_kernel<.., true> for 65; E is no multiple of 64, so the last wave's chunk of
    8 steps ends inside it.  An Inf and a NaN of grad_out sit in features their row's other entries did not win: only
    the winners of those two elements may see them."""
    K = packets * (16 // mr.element_size(dtype))
    c = mr.tiny_case(K, dtype, 'max', True, exact=False, seed=packets)
    big = 1  # the 70-entry row
    c.gout[big, 0], c.gout[big, K - 1] = np.inf, np.nan
    c._ref = None
    d = Dev(c, dev)
    lgG = 6 - min(max(packets - 1, 0).bit_length(), 6)
    for winners in ('records', 'ids32'):
        r = d.route(winners, True)
        assert (r['status'], r['value'], r['sddmm'], r['sddmm_lgG']) == \
            (0, 'masked_sddmm', 'pipelined' if packets <= 64 else 'round4', lgG), (winners, r)
        rec = _records_on_device(c, dev) if winners == 'records' else None
        gv, gm = d.run(winners, True, rec=rec)
        ref = c.ref
        want = np.asarray(ref['gv'], np.float64)
        keep = np.isfinite(want)
        assert (~keep).sum() <= 2 and keep.sum() >= c.E - 2
        got = gv.cpu().double().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), winners
        bound = mr.bound_value(want, ref['gv_l1'], dtype, K)
        bad, ratio = mr.violations(gv.cpu()[keep], ref['gv'][keep], bound[keep], dtype)
        print('masked SDDMM', dtype, packets, winners, 'outside', bad, 'ratio', ratio)
        assert bad == 0


# ---- degenerate shapes -------------------------------------------------------------------------------------------
def test_degenerate_shapes(dev):
    """E = 0, K = 0, M = 0, an empty batch, no column: the entries answer as the route table says, write zeros where an
    output has elements, and nothing outside their outputs.  With both gradients wanted and B N K == 0 while E > 0 the
    pull entries return OK WITHOUT writing grad_value (the open point of docs/design/spmm_backward.md: the masked SDDMM
    is planned, the early exit comes first): pinned here as it stands -- the sentinel survives."""
    i64 = nat._i64
    L = nat.lib()
    P = torch.zeros(64, dtype=torch.int64, device=dev)  # rowptr / col / CSC arrays: empty rows, column 0
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    for dtype in (BF16, F32):
        dt = nat.dtype_code(dtype)
        x = torch.ones(64, dtype=dtype, device=dev)
        for (B, M, N, K, E), gv_state, gm_zero in (((1, 4, 4, 8, 0), 'none', True), ((1, 0, 4, 8, 3), 'zero', True),
                                                   ((0, 4, 4, 8, 3), 'kept', False), ((1, 4, 4, 0, 3), 'kept', False),
                                                   ((1, 4, 0, 8, 3), 'kept', False)):
            ids = torch.full((64, ), E, dtype=torch.int64, device=dev)  # no element has a winner
            ids32 = ids.to(torch.int32)
            for entry in ('ids64', 'ids32', 'records', 'none'):
                gv, gm = Guarded(max(E, 1), dtype, dev), Guarded(max(B * N * K, 1), dtype, dev)
                r = nat.spmm_minmax_bw_route(entry, dtype, B, M, N, K, E, True, True)
                vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
                sizes = (i64(B), i64(M), i64(N), i64(K), i64(E), vp(ws), ctypes.c_size_t(ws.numel()), None)
                if entry == 'none':
                    st = L.tsamd_spmm_minmax_bw(dt, vp(P), vp(P), vp(x), vp(x), vp(x), vp(ids), vp(gv.out), vp(gm.out), *sizes)
                elif entry == 'records':
                    st = L.tsamd_spmm_minmax_bw_csc_records(dt, vp(P), vp(P), 1, vp(x), vp(x), vp(P), vp(P), vp(P), vp(P),
                                                            vp(gv.out), vp(gm.out), *sizes)
                else:
                    fn = L.tsamd_spmm_minmax_bw_csc if entry == 'ids64' else L.tsamd_spmm_minmax_bw_csc_arg32
                    st = fn(dt, vp(P), vp(P), vp(x), vp(x), vp(x), vp(ids if entry == 'ids64' else ids32), vp(P), vp(P), vp(P),
                            vp(gv.out), vp(gm.out), *sizes)
                torch.cuda.synchronize()
                tag = (str(dtype), (B, M, N, K, E), entry)
                assert st == 0 == r['status'], tag
                assert gv.intact() and gm.intact(), tag
                state = gv_state
                if entry == 'none' and state == 'kept':
                    state = 'zero' if B * M * K == 0 else 'rows'  # the scatter entry has no such early exit
                if state == 'zero':
                    assert r['value'] == 'zero' and bool((gv.out[:E] == 0).all()), tag
                elif state == 'kept':
                    assert r['value'] == 'none' and bool((gv.raw == FILL).all()), tag
                if gm_zero:
                    assert r['mat'] == ('scatter' if entry == 'none' and B * M * K > 0 else 'zero'), tag
                    assert bool((gm.out[:B * N * K] == 0).all()), tag
                if B * N * K == 0:
                    assert bool((gm.raw == FILL).all()), tag


@pytest.mark.parametrize('dtype', [BF16, F16])
def test_shadow_shape_with_no_output_row(dev, dtype):
    """M = 0 with an odd B N K (the shape of the fp32 shadow): nothing is added up, so grad_mat is zero-filled where it
    lies -- no workspace is asked for -- and grad_value with it.  (The entry used to clear the shadow, return, and leave
    grad_mat as it found it.)"""
    B, M, N, K, E = 1, 0, 5, 3, 3
    P = torch.zeros(8, dtype=torch.int64, device=dev)
    x = torch.ones(16, dtype=dtype, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for entry in ('none', 'ids64'):
        r = nat.spmm_minmax_bw_route(entry, dtype, B, M, N, K, E, True, True)
        assert (r['status'], r['value'], r['mat'], r['shadow']) == (0, 'zero', 'zero', 0), entry
        gv, gm = Guarded(E, dtype, dev), Guarded(B * N * K, dtype, dev)
        sizes = (nat._i64(B), nat._i64(M), nat._i64(N), nat._i64(K), nat._i64(E), None, ctypes.c_size_t(0), None)
        if entry == 'none':
            st = nat.lib().tsamd_spmm_minmax_bw(nat.dtype_code(dtype), vp(P), vp(P), vp(x), vp(x), vp(x), vp(P), vp(gv.out),
                                                vp(gm.out), *sizes)
        else:
            st = nat.lib().tsamd_spmm_minmax_bw_csc(nat.dtype_code(dtype), vp(P), vp(P), vp(x), vp(x), vp(x), vp(P), vp(P), vp(P),
                                                    vp(P), vp(gv.out), vp(gm.out), *sizes)
        torch.cuda.synchronize()
        assert st == 0 and gv.intact() and gm.intact(), entry
        assert bool((gv.out == 0).all()) and bool((gm.out == 0).all()), entry


# ---- through autograd --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _autograd_case(dtype, K, exact, reduce='max'):
    """few enough entries per row for SparseTensor.matmul to keep records (32 bytes an entry against 12 per element)"""
    route = nat.spmm_route(dtype, 'max', 1, 100, 30002, K, 30000, arg32=True)
    return mr.build_record_forward(K, route, dtype, reduce, True, exact, seed=9, long_rows=(1025, ), long_winners=(65, ))


def _second(arg, M, K):
    if arg.dim() == 1:
        return 'records'
    assert tuple(arg.shape)[-2:] == (M, K)
    return {torch.int64: 'ids64', torch.int32: 'ids32'}[arg.dtype]


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('dtype,K,exact,reduce', [(BF16, 64, True, 'max'), (F32, 128, True, 'min'), (BF16, 36, False, 'max'),
                                                  (F64, 16, False, 'min'), (F16, 128, False, 'min')])
def test_autograd_against_the_oracle(dev, dtype, K, exact, reduce, deterministic):
    """torch.ops.torch_sparse.spmm_min / spmm_max (scatter), torch.ops.tsamd.spmm_minmax in its three forms and
    SparseTensor.matmul, with and without a gradient for the values: outputs and gradients against the host oracle.
    Which route ran is read off the op's second result and storage.has_csr2csc()."""
    import pytorch_sparse_amd as ts
    c = _autograd_case(dtype, K, exact, reduce)
    d = Dev(c, dev)
    is_max = reduce == 'max'
    bare = torch.ops.torch_sparse.spmm_max if is_max else torch.ops.torch_sparse.spmm_min
    es = mr.element_size(dtype)
    packets16 = (K * es) % 16 == 0
    csr, csc = (d.rowptr, d.col), (d.colptr, d.perm, d.row)
    want_out = fr.store(c.forward[0], dtype)
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        for want_value in (False, True):
            def run(op, want_mat=True):
                xr, vr = d.x.clone().requires_grad_(want_mat), d.value.clone().requires_grad_(want_value)
                out, second = op(xr, vr)
                assert bool((fr.bits_of(out) == fr.bits_of(want_out)).all())
                out.backward(d.g)
                return (None if second is None else _second(second, c.M, K)), vr.grad, xr.grad
            tag = (str(dtype), K, want_value, deterministic)
            kind, gv, gm = run(lambda xr, vr: bare(*csr, vr, xr))
            assert kind == 'ids64', tag
            _check(c, gv, gm, exact, 'scatter', tag + ('bare op', ))
            kind, gv, gm = run(lambda xr, vr: torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, is_max, False))
            assert kind == 'ids64', tag
            _check(c, gv, gm, exact, 'pull', tag + ('ids64', ))
            kind, gv, gm = run(lambda xr, vr: torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, is_max, True))
            # records where the forward writes them, they weigh at most three times the ids, and the backward can make
            # grad_value from them; int32 ids otherwise (widened in the backward for the row-parallel kernel)
            light = c.E * mr.record_words(K)[1] * 4 <= 12 * c.M * K
            assert kind == ('records' if dtype != F64 and light and (not want_value or packets16) else 'ids32'), (tag, kind)
            _check(c, gv, gm, exact, 'pull', tag + (kind, ))
            if want_value:
                kind, gv, gm = run(lambda xr, vr: torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, is_max, True), want_mat=False)
                assert kind == 'ids32' and gm is None, tag
                _check(c, gv, None, exact, 'pull', tag + ('grad_value alone', ))
            A = []

            def matmul(xr, vr):
                A.append(ts.SparseTensor(rowptr=csr[0], col=csr[1], value=vr, sparse_sizes=(c.M, c.N), is_sorted=True,
                                         trust_data=True))
                return A[-1].matmul(xr, reduce), None
            _, gv, gm = run(matmul)
            pulled = A[-1].storage.has_csr2csc()
            assert pulled or not deterministic, tag
            _check(c, gv, gm, exact, 'pull' if pulled else 'scatter', tag + ('matmul', 'pull' if pulled else 'scatter'))
    finally:
        torch.use_deterministic_algorithms(before)


@pytest.mark.parametrize('dtype,K,route', [(BF16, 64, 'records'), (F32, 128, 'records'), (F64, 16, 'ids32')])
def test_grad_out_forms(dev, dtype, K, route):
    """grad_out as a stride-0 expansion, with transposed strides and contiguous at an address that is 8 modulo 16, and
    `mat` at 8 modulo 16, with a gradient for the values: on the records route (which realigns the operand: the masked
    SDDMM needs 16-byte packets and there are no ids to fall back on) and on the int32-id route.  All of them give the
    oracle's gradients; the misaligned ones the same bits as the aligned call."""
    c = _autograd_case(dtype, K, False)
    d = Dev(c, dev)
    csr, csc = (d.rowptr, d.col), (d.colptr, d.perm, d.row)
    es = mr.element_size(dtype)

    def off8(t):
        raw = torch.empty(t.numel() * es + 64, dtype=torch.uint8, device=dev)
        start = (8 - raw.data_ptr()) % 16
        v = raw[start:start + t.numel() * es].view(dtype).view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v

    def run(x, g):
        xr, vr = x.requires_grad_(), d.value.clone().requires_grad_()
        out, second = torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, True, True)
        assert _second(second, c.M, K) == route
        out.backward(g)
        return vr.grad, xr.grad

    gv0, gm0 = run(d.x.clone(), d.g)
    _check(c, gv0, gm0, False, 'pull', ('aligned', str(dtype)))
    for name, x, g in (('grad_out at 8 mod 16', d.x.clone(), off8(d.g)), ('mat at 8 mod 16', off8(d.x).detach(), d.g),
                       ('both', off8(d.x).detach(), off8(d.g))):
        gv, gm = run(x, g)
        _check(c, gv, gm, False, 'pull', (name, str(dtype)))
        if route == 'records':
            assert _same_bits(gv, gv0) and _same_bits(gm, gm0), name
    # strided gradients: the op makes them contiguous; the reference follows the values they hold
    keep = c.gout
    try:
        col0 = fr.rounded(np.random.default_rng(3).standard_normal(c.M), dtype if dtype != F64 else F32)
        c.gout, c._ref = np.repeat(col0[:, None], K, axis=1), None
        g = _d(col0, dev, dtype)[:, None].expand(c.M, K)
        assert g.stride() == (1, 0)
        gv, gm = run(d.x.clone(), g)
        _check(c, gv, gm, False, 'pull', ('stride-0 expansion', str(dtype)))
        gt = fr.rounded(np.random.default_rng(4).standard_normal((K, c.M)), dtype if dtype != F64 else F32)
        c.gout, c._ref = np.ascontiguousarray(gt.T), None
        g = _d(gt, dev, dtype).t()
        assert g.stride() == (1, c.M)
        gv, gm = run(d.x.clone(), g)
        _check(c, gv, gm, False, 'pull', ('transposed strides', str(dtype)))
    finally:
        c.gout, c._ref = keep, None


def test_matmul_backward_with_grad_out_at_8_modulo_16(dev):
    """SparseTensor.matmul(x, 'max').backward(g) with trainable values and a contiguous g at 8 modulo 16: the records
    route no longer raises, and returns the oracle's gradients."""
    import pytorch_sparse_amd as ts
    c = _autograd_case(BF16, 128, False)
    d = Dev(c, dev)
    raw = torch.empty(c.M * 128 * 2 + 64, dtype=torch.uint8, device=dev)
    start = (8 - raw.data_ptr()) % 16
    g = raw[start:start + c.M * 128 * 2].view(BF16).view(c.M, 128)
    g.copy_(d.g)
    xr, vr = d.x.clone().requires_grad_(), d.value.clone().requires_grad_()
    A = ts.SparseTensor(rowptr=d.rowptr, col=d.col, value=vr, sparse_sizes=(c.M, c.N), is_sorted=True, trust_data=True)
    out = A.matmul(xr, 'max')
    _, second = torch.ops.tsamd.spmm_minmax(d.rowptr, d.col, d.value, A.storage.colptr(), A.storage.csr2csc(),
                                            A.storage.row(), d.x.clone().requires_grad_(), True, True)
    assert second.dim() == 1, 'the node keeps records for this shape'
    out.backward(g)
    _check(c, vr.grad, xr.grad, False, 'pull', ('matmul, grad_out at 8 mod 16', ))
