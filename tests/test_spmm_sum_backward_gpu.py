"""The sum / mean SpMM backward against the fp64 reference of tests/spmm_grad_reference.py on every kernel route:
the C-ABI value gradient over every lane-group width and trip count of its slot loop (bounded, and bit-exact on
integer inputs), its alignment fallback and degenerate launches; autograd through the bare ops, SparseTensor.matmul
(first / cached backwards, pattern cache off, fixed weights, operand cache), the relabelled layout and the legacy
``spmm(index, value, m, n, x)``; grad_out tensors that are no fresh contiguous buffers; a 200-case fuzz.
Bound everywhere: |got - exact| <= SUM_TOL[T] * L1 + SUM_ATOL[T] (tests/util.py)."""
import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd import synth
from tests import spmm_grad_reference as R
from tests.util import FLOAT_DTYPES, bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ts(dev):
    import pytorch_sparse_amd
    return pytorch_sparse_amd


@pytest.fixture(scope='module')
def ops(ts):
    return torch.ops


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _edge():
    return _cached('edge', R.edge_graph)


def _tiny():
    return _cached('tiny', R.tiny_graphs)


def _misaligned(t):
    """A contiguous tensor with the contents of `t` whose data pointer is one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


# ---- a / b: the C-ABI value gradient over every width ----------------------------------------------------------------
def _sweep(dtype):
    """(K, batch) of both width lists: batch () everywhere, (2,) at 3 / 64 / 65 packets and at K = 7 / 65."""
    vec = 16 // R.element_size(dtype)
    for K in R.vector_widths(dtype):
        yield K, ()
        if K // vec in (3, 64, 65):
            yield K, (2, )
    for K in R.scalar_widths(dtype):
        yield K, ()
        if K in (7, 65):
            yield K, (2, )


def _value_bw_all(dev, G, x, g):
    """{(reduce, row given): result} of the four calls on one (x, g)."""
    row, rp, col = G.row.to(dev), G.rowptr.to(dev), G.col.to(dev)
    xd, gd = x.to(dev), g.to(dev)
    return {(reduce, use_row): nat.spmm_value_bw(row if use_row else None, rp, col, xd, gd, reduce)
            for reduce in ('sum', 'mean') for use_row in (True, False)}


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_value_bw_every_width_against_fp64(dev, dtype):
    G = _edge()
    seen = set()
    for K, batch in _sweep(dtype):
        seen.add(R.value_bw_launch(K, dtype))
        x = synth.features(G.N, K, seed=2, dtype=dtype, batch=batch)
        g = synth.features(G.M, K, seed=3, dtype=dtype, batch=batch)
        got = _value_bw_all(dev, G, x, g)
        for reduce in ('sum', 'mean'):
            exact, l1 = R.grad_value(G.row, G.col, x, g, reduce, G.M)
            for use_row in (True, False):
                R.assert_within_bound(got[reduce, use_row], exact, l1, dtype,
                                      'K=%d batch=%s %s row=%s' % (K, batch, reduce, use_row))
    assert {l for l, _ in seen} == {1, 2, 4, 8, 16, 32, 64} and {t for _, t in seen} == {1, 2, 3}


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_value_bw_every_width_bit_exact_on_integers(dev, dtype):
    G = _edge()
    for K, batch in _sweep(dtype):
        x, g, _ = R.integer_inputs(G, K, dtype, 100 + K, batch)
        got = _value_bw_all(dev, G, x, g)
        exact, l1 = R.grad_value(G.row, G.col, x, g, 'sum', G.M)
        want = exact.to(dtype)
        for use_row in (True, False):
            assert bits_equal(got['sum', use_row], want), 'K=%d batch=%s row=%s' % (K, batch, use_row)
        exact, l1 = R.grad_value(G.row, G.col, x, g, 'mean', G.M)
        for use_row in (True, False):
            R.assert_within_bound(got['mean', use_row], exact, l1, dtype, 'K=%d batch=%s mean' % (K, batch))


# ---- c: alignment fallback ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_value_bw_misaligned_operands_take_the_scalar_kernel(dev, dtype):
    G, K = _edge(), 64
    assert (K * R.element_size(dtype)) % 16 == 0
    row, rp, col = G.row.to(dev), G.rowptr.to(dev), G.col.to(dev)
    for integers in (False, True):
        for batch in ((), (2, )):
            if integers:
                x, g, _ = R.integer_inputs(G, K, dtype, 5, batch)
            else:
                x, g = synth.features(G.N, K, seed=2, dtype=dtype, batch=batch), synth.features(G.M, K, seed=3, dtype=dtype, batch=batch)
            xd, gd = x.to(dev), g.to(dev)
            assert xd.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0
            for reduce in ('sum', 'mean'):
                exact, l1 = R.grad_value(G.row, G.col, x, g, reduce, G.M)
                aligned = nat.spmm_value_bw(row, rp, col, xd, gd, reduce)
                R.assert_within_bound(aligned, exact, l1, dtype, 'aligned')
                for off_x, off_g in ((True, False), (False, True), (True, True)):
                    xm = _misaligned(xd) if off_x else xd
                    gm = _misaligned(gd) if off_g else gd
                    for use_row in (True, False):
                        got = nat.spmm_value_bw(row if use_row else None, rp, col, xm, gm, reduce)
                        tag = '%s x_off=%s g_off=%s batch=%s row=%s' % (reduce, off_x, off_g, batch, use_row)
                        R.assert_within_bound(got, exact, l1, dtype, tag)
                        # equal to the aligned call's within the same bound
                        R.assert_within_bound(got, aligned.cpu().double(), l1, dtype, tag + ' vs aligned')
                        if integers and reduce == 'sum':
                            assert bits_equal(got, aligned) and bits_equal(got, exact.to(dtype)), tag


# ---- d: small and degenerate launches ------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,widths', [(torch.float32, (1, 4, 20, 260)), (torch.bfloat16, (8, 520))])
def test_value_bw_tiny_launches(dev, dtype, widths):
    for G in _tiny():
        for K in widths:
            for batch in ((), (2, )):
                x = synth.features(G.N, K, seed=2, dtype=dtype, batch=batch)
                g = synth.features(G.M, K, seed=3, dtype=dtype, batch=batch)
                got = _value_bw_all(dev, G, x, g)
                for (reduce, use_row), t in got.items():
                    exact, l1 = R.grad_value(G.row, G.col, x, g, reduce, G.M)
                    R.assert_within_bound(t, exact, l1, dtype, 'E=%d K=%d batch=%s %s row=%s' % (
                        G.col.numel(), K, batch, reduce, use_row))
                xi, gi, _ = R.integer_inputs(G, K, dtype, 7, batch)
                exact, _ = R.grad_value(G.row, G.col, xi, gi, 'sum', G.M)
                for (reduce, use_row), t in _value_bw_all(dev, G, xi, gi).items():
                    if reduce == 'sum':
                        assert bits_equal(t, exact.to(dtype)), (G.col.numel(), K, batch, use_row)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_value_bw_degenerate_shapes(dev, dtype):
    G = _tiny()[3]  # 65 entries
    E = G.col.numel()
    row, rp, col = G.row.to(dev), G.rowptr.to(dev), G.col.to(dev)
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    rp0 = torch.zeros(G.M + 1, dtype=torch.int64, device=dev)
    for reduce in ('sum', 'mean'):
        for use_row in (True, False):
            # no entries
            x, g = synth.features(G.N, 8, seed=2, dtype=dtype).to(dev), synth.features(G.M, 8, seed=3, dtype=dtype).to(dev)
            out = nat.spmm_value_bw(empty if use_row else None, rp0, empty, x, g, reduce)
            assert out.dtype == dtype and tuple(out.shape) == (0, )
            # no features
            x0 = torch.zeros(G.N, 0, dtype=dtype, device=dev)
            g0 = torch.zeros(G.M, 0, dtype=dtype, device=dev)
            out = nat.spmm_value_bw(row if use_row else None, rp, col, x0, g0, reduce)
            assert out.dtype == dtype and tuple(out.shape) == (E, ) and bool((out == 0).all())
            # an empty batch
            xb = torch.zeros(0, G.N, 8, dtype=dtype, device=dev)
            gb = torch.zeros(0, G.M, 8, dtype=dtype, device=dev)
            out = nat.spmm_value_bw(row if use_row else None, rp, col, xb, gb, reduce)
            assert out.dtype == dtype and tuple(out.shape) == (E, ) and bool((out == 0).all())


# ---- e: autograd, every route ----------------------------------------------------------------------------------------
AUTOGRAD_WIDTHS = {torch.float32: (1, 7, 32, 33, 64, 130), torch.bfloat16: (1, 7, 32, 33, 64, 130),
                   torch.float16: (7, 64), torch.float64: (7, 64)}
MODES = ('trainable', 'fixed', 'none')


class _Case:
    """One (dtype, K, batch, value mode) on the edge graph: device inputs and the cached fp64 references."""

    def __init__(self, dev, dtype, K, batch, mode, G=None, integers=False):
        self.G = G = _edge() if G is None else G
        self.dev, self.dtype, self.K, self.batch, self.mode, self.integers = dev, dtype, K, batch, mode, integers
        E = G.col.numel()
        if integers:
            self.x, self.g, self.v = R.integer_inputs(G, K, dtype, 50 + K, batch, with_value=mode != 'none')
        else:
            self.x, self.g = synth.features(G.N, K, seed=2, dtype=dtype, batch=batch), synth.features(G.M, K, seed=3, dtype=dtype, batch=batch)
            self.v = None if mode == 'none' else R.edge_values(E, dtype)
        self.row, self.rowptr, self.col = G.row.to(dev), G.rowptr.to(dev), G.col.to(dev)
        self.gd = self.g.to(dev)
        self.tag = '%s K=%d batch=%s values=%s' % (dtype, K, batch, mode)

    def leaves(self):
        """Fresh (value, x) on the device with the gradient flags of the mode."""
        x = self.x.to(self.dev).requires_grad_()
        v = None if self.v is None else self.v.to(self.dev)
        if self.mode == 'trainable':
            v.requires_grad_()
        return v, x

    def ref(self, reduce, scale=1):
        key = ('ref', id(self.G), self.dtype, self.K, self.batch, self.mode != 'none', self.integers, reduce, scale)
        v = self.v if self.v is None or scale == 1 else self.v * scale  # (rounded to the dtype, as mul_ does)
        return _cached(key, lambda: R.reference(self.G.row, self.G.col, v, self.x, self.g, reduce, self.G.M))

    def tensor(self, ts, v):
        return ts.SparseTensor(rowptr=self.rowptr, col=self.col, value=v, sparse_sizes=(self.G.M, self.G.N),
                               is_sorted=True, trust_data=True)

    def check(self, what, reduce, out, v, x, scale=1):
        ref, dtype, tag = self.ref(reduce, scale), self.dtype, '%s %s %s' % (self.tag, reduce, what)
        assert out.dtype == dtype and x.grad is not None and x.grad.dtype == dtype, tag
        if self.integers:
            assert bits_equal(out, ref.out.to(dtype)), tag + ' out'
            assert bits_equal(x.grad, ref.grad_mat.to(dtype)), tag + ' grad_mat'
        else:
            R.assert_within_bound(out, ref.out, ref.out_l1, dtype, tag + ' out')
            R.assert_within_bound(x.grad, ref.grad_mat, ref.grad_mat_l1, dtype, tag + ' grad_mat')
        assert bool((x.grad[..., self.G.unreferenced.to(self.dev), :] == 0).all()), tag + ' unreferenced columns'
        if self.mode == 'trainable':
            assert v.grad is not None and v.grad.dtype == dtype and tuple(v.grad.shape) == tuple(v.shape), tag
            if self.integers:
                assert bits_equal(v.grad, ref.grad_value.to(dtype)), tag + ' grad_value'
            else:
                R.assert_within_bound(v.grad, ref.grad_value, ref.grad_value_l1, dtype, tag + ' grad_value')
        elif v is not None:
            assert v.grad is None, tag


def _cases(dev, dtype, modes=MODES):
    for K in AUTOGRAD_WIDTHS[dtype]:
        for batch in ((), (2, )):
            for mode in modes:
                yield _Case(dev, dtype, K, batch, mode)


def _bare(ops, case, reduce, v, x, csc=None):
    colptr, perm = csc if csc is not None else _cached(('csc', id(case.G), str(case.dev)), lambda: tuple(
        t.to(case.dev) for t in R.csc_arrays(case.G)))
    if reduce == 'sum':
        return ops.torch_sparse.spmm_sum(case.row, case.rowptr, case.col, v, colptr, perm, x)
    rowcount = case.rowptr[1:] - case.rowptr[:-1]
    return ops.torch_sparse.spmm_mean(case.row, case.rowptr, case.col, v, rowcount, colptr, perm, x)


def _pattern_cache_delta(ops, before):
    """[backwards served from the kept CSC row ids, from the kept value[csr2csc], gathers of value[csr2csc]] since."""
    return [b - a for a, b in zip(before[1:], ops.tsamd.pattern_cache_stats()[1:])]


def _expected_route(case, reduce, i, cache_on=True, refreshed=False):
    """What backward #i on one SparseTensor does with the transposed-pattern cache (ops_spmm_state.cpp): #0 meets a new
    pattern and reads through csr2csc; from #1 on the kept row ids serve; fixed weights of a sum are gathered into
    the entry at #1 (and again after an in-place update), then served from it."""
    if not cache_on or i == 0:
        return [0, 0, 0]
    fixed_sum = case.mode == 'fixed' and reduce == 'sum'
    fill = fixed_sum and (i == 1 or refreshed)
    return [1, 1 if fixed_sum and not fill else 0, 1 if fill else 0]


def _matmul_rounds(ts, ops, case, reduce, rounds, what, cache_on=True):
    """`rounds` forward + backward passes on ONE SparseTensor, each held to the reference; the route every backward
    took is read from the pattern cache's counters, not assumed."""
    v, x = case.leaves()
    A = case.tensor(ts, v)
    for i in range(rounds):
        x.grad = None
        if v is not None:
            v.grad = None
        out = A.matmul(x, reduce)
        before = ops.tsamd.pattern_cache_stats()
        out.backward(case.gd)
        assert _pattern_cache_delta(ops, before) == _expected_route(case, reduce, i, cache_on), \
            '%s %s %s #%d' % (case.tag, reduce, what, i)
        case.check('%s #%d' % (what, i), reduce, out.detach(), v, x)
    return A, v, x


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_autograd_bare_ops(dev, ops, dtype):
    for case in _cases(dev, dtype):
        for reduce in ('sum', 'mean'):
            v, x = case.leaves()
            out = _bare(ops, case, reduce, v, x)
            out.backward(case.gd)
            case.check('bare op', reduce, out.detach(), v, x)


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_autograd_matmul_first_and_cached_backwards(dev, ts, ops, dtype):
    assert ops.tsamd.pattern_cache(True), 'the pattern cache is on by default'
    for case in _cases(dev, dtype):
        for reduce in ('sum', 'mean'):
            _matmul_rounds(ts, ops, case, reduce, 3, 'matmul')


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_autograd_matmul_without_pattern_cache(dev, ts, ops, dtype):
    was = ops.tsamd.pattern_cache(False)
    try:
        for case in _cases(dev, dtype):
            for reduce in ('sum', 'mean'):
                _matmul_rounds(ts, ops, case, reduce, 3, 'matmul, pattern cache off', cache_on=False)
    finally:
        ops.tsamd.pattern_cache(was)


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_autograd_fixed_weights_and_their_update(dev, ts, ops, dtype):
    assert ops.tsamd.pattern_cache(True)
    for case in _cases(dev, dtype, modes=('fixed', )):
        for reduce in ('sum', 'mean'):
            A, v, x = _matmul_rounds(ts, ops, case, reduce, 4, 'fixed weights')
            v.mul_(3)
            assert bits_equal(v, case.v * 3)
            x.grad = None
            out = A.matmul(x, reduce)
            before = ops.tsamd.pattern_cache_stats()
            out.backward(case.gd)
            assert _pattern_cache_delta(ops, before) == _expected_route(case, reduce, 4, refreshed=True), case.tag
            case.check('fixed weights after mul_(3)', reduce, out.detach(), v, x, scale=3)


def test_pattern_cache_entry_belongs_to_one_stream(dev, ts, ops):
    """The stream is part of the pattern cache's key: a backward on another stream starts a new entry (a first
    sighting, then the gathers of the second), and so does the next one back on the original stream -- the single entry
    was replaced.  Every round is held to the fp64 reference."""
    assert ops.tsamd.pattern_cache(True)
    case = _Case(dev, torch.float32, 7, (), 'fixed')
    v, x = case.leaves()
    A = case.tensor(ts, v)
    seen = []

    def one_round(what, sighting):
        x.grad = None
        out = A.matmul(x, 'sum')
        before = ops.tsamd.pattern_cache_stats()
        out.backward(case.gd)
        seen.append(_pattern_cache_delta(ops, before))
        assert seen[-1] == _expected_route(case, 'sum', sighting), '%s %s sighting #%d' % (case.tag, what, sighting)
        case.check('%s sighting #%d' % (what, sighting), 'sum', out.detach(), v, x)

    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    for i in range(2):
        one_round('first stream', i)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        for i in range(2):
            one_round('side stream', i)
    main.wait_stream(side)
    one_round('back on the first stream', 0)
    assert seen == [[0, 0, 0], [1, 0, 1], [0, 0, 0], [1, 0, 1], [0, 0, 0]]


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_autograd_relabelled_layout(dev, ts, dtype):
    for case in _cases(dev, dtype):
        for reduce in ('sum', 'mean'):
            v, x = case.leaves()
            A = case.tensor(ts, v)
            out = ts.from_relabelled(ts.matmul_relabelled(A, ts.to_relabelled(x), reduce))
            out.backward(case.gd)
            case.check('relabelled', reduce, out.detach(), v, x)


@pytest.mark.parametrize('dtype,reduce', [(torch.float32, 'sum'), (torch.float32, 'mean'), (torch.bfloat16, 'mean'),
                                          (torch.float16, 'sum'), (torch.float64, 'sum')])
def test_autograd_with_operand_cache(dev, ts, ops, dtype, reduce):
    """The forward through tsamd_spmm_cached.  The cache only engages where the forward would copy its dense operand
    (2^20 entries and up, rows of a power-of-two size >= 256 bytes): cache_graph() at cache_width(dtype) is the
    smallest such problem -- the edge graph never reaches this route.  The counters show one fill and one hit; the
    forward and both gradients of BOTH passes are held to the fp64 reference."""
    G = _cached('cache_graph', R.cache_graph)
    case = _Case(dev, dtype, R.cache_width(dtype), (), 'trainable', G=G)
    was = ops.tsamd.operand_cache(False)[0]
    try:
        _, hits0, fills0 = ops.tsamd.operand_cache(True)
        v, x = case.leaves()
        A = case.tensor(ts, v)
        for i in range(2):
            x.grad = v.grad = None
            out = A.matmul(x, reduce)
            out.backward(case.gd)
            case.check('operand cache #%d' % i, reduce, out.detach(), v, x)
        _, hits1, fills1 = ops.tsamd.operand_cache(True)
        assert (fills1 - fills0, hits1 - hits0) == (1, 1), (hits0, fills0, hits1, fills1)
    finally:
        ops.tsamd.operand_cache(bool(was))


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_autograd_bit_exact_on_integers(dev, ts, ops, dtype):
    for K in (33, 64):
        for batch in ((), (2, )):
            for mode in ('trainable', 'none'):
                case = _Case(dev, dtype, K, batch, mode, integers=True)
                _matmul_rounds(ts, ops, case, 'sum', 2, 'integers, matmul')
                v, x = case.leaves()
                out = _bare(ops, case, 'sum', v, x)
                out.backward(case.gd)
                case.check('integers, bare op', 'sum', out.detach(), v, x)


# ---- f: forms of grad_out ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,K', [(torch.float32, 64), (torch.bfloat16, 8)])
@pytest.mark.parametrize('reduce', ['sum', 'mean'])
def test_grad_out_forms(dev, ts, ops, dtype, K, reduce):
    G = _edge()
    for batch in ((), (2, )):
        base = _Case(dev, dtype, K, batch, 'trainable')
        for route in ('bare', 'matmul'):
            def product(v, x):
                return _bare(ops, base, reduce, v, x) if route == 'bare' else base.tensor(ts, v).matmul(x, reduce)

            def held_to(g, out, v, x, what):
                ref = R.reference(G.row, G.col, base.v, base.x, g, reduce, G.M)
                tag = '%s %s %s %s' % (base.tag, reduce, route, what)
                R.assert_within_bound(out, ref.out, ref.out_l1, dtype, tag + ' out')
                R.assert_within_bound(v.grad, ref.grad_value, ref.grad_value_l1, dtype, tag + ' grad_value')
                R.assert_within_bound(x.grad, ref.grad_mat, ref.grad_mat_l1, dtype, tag + ' grad_mat')

            # 1. out.sum(): the engine hands over a stride-0 expansion of one element
            v, x = base.leaves()
            out = product(v, x)
            out.sum().backward()
            held_to(torch.ones(*batch, G.M, K, dtype=dtype), out.detach(), v, x, 'sum()')
            # 2. a consumer of the transpose: grad_out arrives with the strides of a transposed tensor
            w = synth.features(K, G.M, seed=17, dtype=dtype, batch=batch)
            v, x = base.leaves()
            out = product(v, x)
            (out.transpose(-1, -2) * w.to(dev)).sum().backward()
            held_to(w.transpose(-1, -2).contiguous(), out.detach(), v, x, 'transposed consumer')
            # 3. a contiguous grad_out whose data pointer is not 16-byte aligned
            v, x = base.leaves()
            out = product(v, x)
            out.backward(_misaligned(base.gd))
            held_to(base.g, out.detach(), v, x, 'misaligned grad_out')


# ---- g: the legacy spmm(index, value, m, n, x) under autograd ---------------------------------------------------------
def _legacy_coo(m, n, E, dup, seed, sort):
    rs = np.random.RandomState(seed)
    key = rs.choice(m * n, E - dup, replace=False)
    key = np.concatenate([key, rs.choice(key, dup, replace=False)]) if dup else key
    key = np.sort(key) if sort else key[rs.permutation(key.size)]
    index = torch.from_numpy(np.stack([key // n, key % n])).long()
    if key.size > 1 and not sort:
        assert bool(((index[0, 1:] * n + index[1, 1:]) < (index[0, :-1] * n + index[1, :-1])).any()), 'unsorted'
    assert np.unique(key).size == key.size - dup
    return index


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('K', [1, 16, 33])
def test_legacy_spmm_gradients(dev, ts, dtype, K):
    m, n = 200, 150
    for name, index in (('unsorted, 10 % duplicates', _legacy_coo(m, n, 3000, 300, 1, False)),
                        ('sorted', _legacy_coo(m, n, 3000, 300, 2, True)),
                        ('one entry', _legacy_coo(m, n, 1, 0, 3, False)),
                        ('no entry', _legacy_coo(m, n, 0, 0, 4, False))):
        E = index.size(1)
        value = R.edge_values(E, dtype, 5)
        x = synth.features(n, K, seed=6, dtype=dtype)
        g = synth.features(m, K, seed=7, dtype=dtype)
        ref = R.reference(index[0], index[1], value, x, g, 'sum', m)
        v, xd = value.to(dev).requires_grad_(), x.to(dev).requires_grad_()
        out = ts.spmm(index.to(dev), v, m, n, xd)
        out.backward(g.to(dev))
        tag = '%s %s K=%d' % (name, dtype, K)
        assert tuple(out.shape) == (m, K) and tuple(v.grad.shape) == (E, ) and tuple(xd.grad.shape) == (n, K), tag
        R.assert_within_bound(out.detach(), ref.out, ref.out_l1, dtype, tag + ' out')
        R.assert_within_bound(v.grad, ref.grad_value, ref.grad_value_l1, dtype, tag + ' grad_value')
        R.assert_within_bound(xd.grad, ref.grad_mat, ref.grad_mat_l1, dtype, tag + ' grad_mat')


# ---- h: fuzz -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', range(4))
def test_sum_mean_backward_fuzz(dev, ops, chunk):
    """4 x 50 random small problems with the shapes of test_spmm_fuzz_small_shapes (ragged, empty leading / trailing
    rows, rows ending on partition boundaries, heavy rows, batches) through the bare ops, both gradients."""
    rng = np.random.RandomState(4321 + chunk)
    for case in range(50):
        M = int(rng.choice([1, 2, 3, 7, 64, 129, 500, 1025]))
        N = int(rng.choice([1, 2, 5, 33, 128, 1000]))
        kind = rng.randint(4)
        if kind == 0:
            deg = rng.randint(0, 6, size=M)
        elif kind == 1:
            deg = rng.choice([0, 63, 64, 65, 127, 128], size=M)
        elif kind == 2:
            deg = np.zeros(M, dtype=np.int64)
            deg[rng.randint(M)] = int(rng.choice([1, 64, 1000, 5000]))
        else:
            deg = np.where(np.arange(M) < max(1, M // 4), rng.randint(0, 300, size=M), 0)
        rp = torch.zeros(M + 1, dtype=torch.int64)
        rp[1:] = torch.from_numpy(np.cumsum(deg))
        E = int(rp[-1])
        col = torch.from_numpy(rng.randint(0, N, size=E)).long()
        row = torch.repeat_interleave(torch.arange(M), rp[1:] - rp[:-1])
        dtype = FLOAT_DTYPES[rng.randint(4)]
        K = int(rng.choice([1, 2, 3, 4, 8, 12, 16, 33, 64, 100, 130]))
        batch = () if rng.rand() < 0.7 else (int(rng.randint(1, 4)), )
        has_value = bool(rng.rand() < 0.6)
        reduce = ['sum', 'mean'][rng.randint(2)]
        seed = 1000 * chunk + case
        value = R.edge_values(E, dtype, seed) if has_value else None
        x = synth.features(N, K, seed=seed + 1, dtype=dtype, batch=batch)
        g = synth.features(M, K, seed=seed + 2, dtype=dtype, batch=batch)
        G = R.Graph(row, col, rp, M, N, -1, -1, None)
        colptr, perm = R.csc_arrays(G)
        v = None if value is None else value.to(dev).requires_grad_()
        xd = x.to(dev).requires_grad_()
        args = (row.to(dev), rp.to(dev), col.to(dev), v)
        if reduce == 'sum':
            out = ops.torch_sparse.spmm_sum(*args, colptr.to(dev), perm.to(dev), xd)
        else:
            out = ops.torch_sparse.spmm_mean(*args, (rp[1:] - rp[:-1]).to(dev), colptr.to(dev), perm.to(dev), xd)
        out.backward(g.to(dev))
        ref = R.reference(row, col, value, x, g, reduce, M)
        try:
            R.assert_within_bound(out.detach(), ref.out, ref.out_l1, dtype, 'out')
            R.assert_within_bound(xd.grad, ref.grad_mat, ref.grad_mat_l1, dtype, 'grad_mat')
            if has_value:
                R.assert_within_bound(v.grad, ref.grad_value, ref.grad_value_l1, dtype, 'grad_value')
        except AssertionError as exc:
            raise AssertionError('chunk %d case %d: M=%d N=%d E=%d K=%d %s %s batch=%s value=%s kind=%d: %s' % (
                chunk, case, M, N, E, K, dtype, reduce, batch, has_value, kind, exc))
