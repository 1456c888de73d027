"""Value gradients of the sparse-sparse product (csrc/spspmm_bw.hip, the autograd node of tsamd::spspmm) against the
fp64 oracle of tests/spspmm_grad_reference.py, whose census (tests/test_spspmm_grad_reference.py, no GPU) proves that
every builder reaches its route.  'dyadic' values: the bits of the exact result; 'uniform': within the project's
SUM_TOL * L1 + SUM_ATOL.  On the code before this feature every public-path test raises "does not require grad" and
the C-ABI tests fail on the missing symbols."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import SparseTensor, matmul
from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd.matmul import spspmm as spspmm_tensor
from pytorch_sparse_amd.spspmm import spspmm as spspmm_functional
from tests import spspmm_grad_reference as R

pytestmark = pytest.mark.gpu

TORCH_DT = {'f32': torch.float32, 'f64': torch.float64}
NAMES = ('long_row', 'tall_col', 'aligned', 'empties', 'wide', 'unstaged')


def route_words():
    return nat.spspmm_bw_route(torch.float32)


@functools.lru_cache(maxsize=None)
def lg_range(dtype):
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_spspmm_route(0 if dtype == 'f32' else 1, ctypes.c_int64(2 ** 32 - 2), out) == 0
    return int(out[0])


def get_cases(dtype):
    w = route_words()
    return R.builders(w[0], w[1], lg_range(dtype))


def expected(name, kind, dtype, mode):
    w = route_words()
    return R.expected(w[0], w[1], lg_range(dtype), name, kind, dtype, mode)


def t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def dev_case(name, dtype, dev):
    c = get_cases(dtype)[name]
    keys = ('rowptrA', 'colA', 'rowptrB', 'colB', 'rowptrC', 'colC', 'colptrA', 'csr2cscA', 'rowA')
    d = {k: t(c[k], dev) for k in keys}
    d['rowA_t'] = d['rowA'][d['csr2cscA']]
    return d


def _misaligned(x):
    """A contiguous tensor with the contents of `x` whose data pointer is one element past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def cabi(d, side, va, vb, g, misaligned=False):
    """One side through the C-ABI, into a buffer of NaNs (every element has to be written by the call)."""
    dev = g.device
    if misaligned:
        g = _misaligned(g)
    if side == 0:
        grad = torch.full((d['colA'].numel(), ), float('nan'), dtype=g.dtype, device=dev)
        out, P = nat.spspmm_value_bw(0, d['rowptrA'], d['colA'], d['rowptrB'], d['colB'], vb, d['rowptrC'], d['colC'], g,
                                     grad)
    else:
        grad = torch.full((d['colB'].numel(), ), float('nan'), dtype=g.dtype, device=dev)
        va_t = None if va is None else va[d['csr2cscA']].contiguous()
        out, P = nat.spspmm_value_bw(1, d['rowptrB'], d['colB'], d['colptrA'], d['rowA_t'], va_t, d['rowptrC'],
                                     d['colC'], g, grad)
    torch.cuda.synchronize()
    return out.cpu().numpy(), P


# ---- C-ABI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name', NAMES)
def test_cabi_both_sides_against_the_oracle(dev, name, dtype):
    d = dev_case(name, dtype, dev)
    case = get_cases(dtype)[name]
    for kind in ('dyadic', 'uniform'):
        for mode in ('both', 'a_only', 'b_only'):  # the value-less other side counts as all ones
            va, vb, g, gA, gB, l1A, l1B = expected(name, kind, dtype, mode)
            tva, tvb, tg = t(va, dev), t(vb, dev), t(g, dev)
            gotA, P = cabi(d, 0, tva, tvb, tg)
            assert P == case['prodA'].size
            ra = R.check_grad(gotA, gA, l1A, dtype, kind, '%s gA %s %s' % (name, kind, mode))
            gotB, P = cabi(d, 1, tva, tvb, tg)
            assert P == case['prodA'].size
            rb = R.check_grad(gotB, gB, l1B, dtype, kind, '%s gB %s %s' % (name, kind, mode))
            print('SPSPMM-BW %s %s %s %s err/bound gA=%.3g gB=%.3g' % (name, dtype, kind, mode, ra, rb))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_cabi_misaligned_gc(dev, dtype):
    d = dev_case('long_row', dtype, dev)
    for kind in ('dyadic', 'uniform'):
        va, vb, g, gA, gB, l1A, l1B = expected('long_row', kind, dtype, 'both')
        tva, tvb, tg = t(va, dev), t(vb, dev), t(g, dev)
        for side, exact, l1 in ((0, gA, l1A), (1, gB, l1B)):
            got, _ = cabi(d, side, tva, tvb, tg, misaligned=True)
            R.check_grad(got, exact, l1, dtype, kind, 'misaligned side %d' % side)
            same, _ = cabi(d, side, tva, tvb, tg)
            assert np.array_equal(R.stored(got, dtype).view(np.uint8), R.stored(same, dtype).view(np.uint8))


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['long_row', 'tall_col'])
def test_two_calls_return_equal_bits(dev, name, dtype):
    d = dev_case(name, dtype, dev)
    va, vb, g, *_ = expected(name, 'uniform', dtype, 'both')
    tva, tvb, tg = t(va, dev), t(vb, dev), t(g, dev)
    for side in (0, 1):
        a, _ = cabi(d, side, tva, tvb, tg)
        b, _ = cabi(d, side, tva, tvb, tg)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), 'side %d' % side


def _pair_on(dev, case):
    keys = ('rowptrA', 'colA', 'rowptrB', 'colB', 'rowptrC', 'colC', 'colptrA', 'csr2cscA', 'rowA')
    d = {k: t(case[k], dev) for k in keys}
    d['rowA_t'] = d['rowA'][d['csr2cscA']]
    return d


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_degenerate_launches_write_zeros(dev, dtype):
    b_rows = [[0, 2], [], [1, 3, 4]]
    pairs = {
        'M = 0': R.make_pair('m0', [], b_rows, 5),
        'nnzA = 0': R.make_pair('a0', [[], []], b_rows, 5),
        'nnzB = 0': R.make_pair('b0', [[0, 1], [2]], [[], [], []], 5),
        'P = 0': R.make_pair('p0', [[1], [], [1]], b_rows, 5),
    }
    for tag, case in pairs.items():
        assert case['prodA'].size == 0 and case['colC'].size == 0, tag
        d = _pair_on(dev, case)
        g = torch.zeros(0, dtype=TORCH_DT[dtype], device=dev)
        for mode in ('both', 'none'):
            va = torch.ones(case['colA'].size, dtype=g.dtype, device=dev) if mode == 'both' else None
            vb = torch.ones(case['colB'].size, dtype=g.dtype, device=dev) if mode == 'both' else None
            for side, n in ((0, case['colA'].size), (1, case['colB'].size)):
                got, P = cabi(d, side, va, vb, g)
                assert P == 0 and got.shape == (n, ) and not got.any(), '%s side %d' % (tag, side)


def test_other_dtypes_are_unsupported(dev):
    L = nat.lib()
    z = ctypes.c_void_p(0)
    i0 = ctypes.c_int64(0)
    for dt in (2, 3, 4, 5):  # fp16, bf16, int32, int64
        assert L.tsamd_spspmm_bw_plan(dt, 0, z, i0, z, i0, z, z, z, z, ctypes.c_size_t(0), z) == 2
        assert L.tsamd_spspmm_value_bw(dt, 0, z, i0, z, i0, z, i0, z, z, z, z, z, z, z, z, ctypes.c_size_t(0), z) == 2
    assert L.tsamd_spspmm_value_bw(0, 2, z, i0, z, i0, z, i0, z, z, z, z, z, z, z, z, ctypes.c_size_t(0), z) == 1


# ---- public paths --------------------------------------------------------------------------------------------------
def _random_case(seed):
    rng = np.random.default_rng(seed)
    m, k, n = 60, 50, 70
    a = [np.nonzero(rng.random(k) < 0.12)[0] for _ in range(m)]
    b = [np.nonzero(rng.random(n) < 0.12)[0] for _ in range(k)]
    a[0], a[7], b[4] = [], [], []
    return R.make_pair('random', a, b, n)


@functools.lru_cache(maxsize=None)
def public_case(which):
    return get_cases('f32')['long_row'] if which == 'long_row' else _random_case(3)


def _tensor_path(case, dev, cached_csc):
    def run(va, vb):
        A = SparseTensor(rowptr=t(case['rowptrA'], dev), col=t(case['colA'], dev), value=va,
                         sparse_sizes=(case['m'], case['k']), is_sorted=True, trust_data=True)
        B = SparseTensor(rowptr=t(case['rowptrB'], dev), col=t(case['colB'], dev), value=vb,
                         sparse_sizes=(case['k'], case['N']), is_sorted=True, trust_data=True)
        if cached_csc:
            A.storage.colptr()
            A.storage.csr2csc()
            assert A.storage._colptr is not None and A.storage._csr2csc is not None
        C = A @ B
        rp, col, val = C.csr()
        return rp, col, val
    return run, None, None


def _functional_path(case, dev, shuffled):
    """-> (run, permA, permB): run(va, vb) takes the values in the ORDER OF THE INPUT INDEX (shuffled or not)."""
    ia = np.stack([case['rowA'], case['colA']])
    ib = np.stack([case['rowB'], case['colB']])
    pa = pb = None
    if shuffled:
        rng = np.random.default_rng(5)
        pa, pb = rng.permutation(ia.shape[1]), rng.permutation(ib.shape[1])
        ia, ib = ia[:, pa], ib[:, pb]
    tia, tib = t(ia, dev), t(ib, dev)

    def run(va, vb):
        idx, val = spspmm_functional(tia, va, tib, vb, case['m'], case['k'], case['N'], coalesced=shuffled)
        rp = torch.ops.torch_sparse.ind2ptr(idx[0], case['m'])
        return rp, idx[1], val
    return run, pa, pb


PATHS = ['tensor', 'tensor_cached_csc', 'functional', 'functional_shuffled']


def make_path(path, case, dev):
    if path.startswith('tensor'):
        return _tensor_path(case, dev, path.endswith('cached_csc'))
    return _functional_path(case, dev, path.endswith('shuffled'))


def _leaf(a, perm, dtype, dev, requires_grad=True):
    a = a if perm is None else a[perm]
    return t(a.astype(R.NP_DT[dtype]), dev).requires_grad_(requires_grad)


def _grad_np(x, perm):
    """.grad of a leaf, back in the operand's own entry order."""
    g = x.grad.detach().cpu().numpy()
    if perm is None:
        return g
    out = np.empty_like(g)
    out[perm] = g
    return out


@pytest.mark.parametrize('which', ['random', 'long_row'])
@pytest.mark.parametrize('path', PATHS)
def test_public_paths(dev, path, which):
    case = public_case(which)
    run, pa, pb = make_path(path, case, dev)
    va64, vb64, g64 = R.values(case, 'uniform', 1)
    for dtype in ('f32', 'f64'):
        va_s, vb_s, g_s = (R.stored(x, dtype) for x in (va64, vb64, g64))
        f64 = lambda a: a.astype(np.float64)  # noqa: E731
        # a random gC; the pattern is the oracle's
        va, vb = _leaf(va_s, pa, dtype, dev), _leaf(vb_s, pb, dtype, dev)
        rp, col, val = run(va, vb)
        assert np.array_equal(rp.cpu().numpy(), case['rowptrC']) and np.array_equal(col.cpu().numpy(), case['colC'])
        assert val.requires_grad and val.dtype == TORCH_DT[dtype] and not rp.requires_grad and not col.requires_grad
        val.backward(t(g_s, dev), retain_graph=True)
        gA, gB, l1A, l1B = R.oracle(case, f64(va_s), f64(vb_s), f64(g_s))
        first = (_grad_np(va, pa), _grad_np(vb, pb))
        R.check_grad(first[0], gA, l1A, dtype, 'uniform', '%s gA' % path)
        R.check_grad(first[1], gB, l1B, dtype, 'uniform', '%s gB' % path)
        # the same graph again: identical bits
        va.grad = vb.grad = None
        val.backward(t(g_s, dev))
        assert np.array_equal(first[0].view(np.uint8), _grad_np(va, pa).view(np.uint8))
        assert np.array_equal(first[1].view(np.uint8), _grad_np(vb, pb).view(np.uint8))
        # valueC.sum().backward(): grad_out is a stride-0 expand
        ones = np.ones_like(g_s)
        gA1, gB1, l1A1, l1B1 = R.oracle(case, f64(va_s), f64(vb_s), f64(ones))
        va, vb = _leaf(va_s, pa, dtype, dev), _leaf(vb_s, pb, dtype, dev)
        run(va, vb)[2].sum().backward()
        R.check_grad(_grad_np(va, pa), gA1, l1A1, dtype, 'uniform', '%s gA of sum' % path)
        R.check_grad(_grad_np(vb, pb), gB1, l1B1, dtype, 'uniform', '%s gB of sum' % path)
        # one side only
        va, vb = _leaf(va_s, pa, dtype, dev), _leaf(vb_s, pb, dtype, dev, requires_grad=False)
        run(va, vb)[2].backward(t(g_s, dev))
        assert vb.grad is None
        R.check_grad(_grad_np(va, pa), gA, l1A, dtype, 'uniform', '%s only A' % path)
        va, vb = _leaf(va_s, pa, dtype, dev, requires_grad=False), _leaf(vb_s, pb, dtype, dev)
        run(va, vb)[2].backward(t(g_s, dev))
        assert va.grad is None
        R.check_grad(_grad_np(vb, pb), gB, l1B, dtype, 'uniform', '%s only B' % path)


@pytest.mark.parametrize('path', PATHS)
def test_public_paths_mixed_dtypes_and_double_backward(dev, path):
    case = public_case('random')
    run, pa, pb = make_path(path, case, dev)
    va64, vb64, g64 = R.values(case, 'dyadic', 2)
    # fp32 A with fp64 B: the product is fp64, each .grad has its operand's dtype; dyadic -> exact bits
    va, vb = _leaf(va64, pa, 'f32', dev), _leaf(vb64, pb, 'f64', dev)
    val = run(va, vb)[2]
    assert val.dtype == torch.float64
    val.backward(t(g64, dev))
    gA, gB, l1A, l1B = R.oracle(case, va64, vb64, g64)
    assert va.grad.dtype == torch.float32 and vb.grad.dtype == torch.float64
    R.check_grad(_grad_np(va, pa), gA, l1A, 'f32', 'dyadic', '%s mixed gA' % path)
    R.check_grad(_grad_np(vb, pb), gB, l1B, 'f64', 'dyadic', '%s mixed gB' % path)
    # first order only: the gradient carries no graph, a double backward raises instead of returning zeros
    va, vb = _leaf(va64, pa, 'f64', dev), _leaf(vb64, pb, 'f64', dev)
    val = run(va, vb)[2]
    ga, gb = torch.autograd.grad(val.sum(), [va, vb], create_graph=True)
    assert not ga.requires_grad and not gb.requires_grad
    with pytest.raises(RuntimeError, match='does not require grad'):
        (ga.sum() + gb.sum()).backward()


@pytest.mark.parametrize('path', ['tensor', 'functional'])
def test_one_sided_requests_and_value_less_operands(dev, path):
    """torch.autograd.grad for one of two leaves that both require grad (the node computes that side alone), and an
    operand without values (all ones, no gradient; the other side's edge moves up by one)."""
    case = public_case('random')
    run, _, _ = make_path(path, case, dev)
    va64, vb64, g64 = R.values(case, 'dyadic', 7)
    tg = t(g64, dev)
    gA, gB, l1A, l1B = R.oracle(case, va64, vb64, g64)
    va, vb = _leaf(va64, None, 'f64', dev), _leaf(vb64, None, 'f64', dev)
    val = run(va, vb)[2]
    (ga, ) = torch.autograd.grad(val, [va], tg, retain_graph=True)
    (gb, ) = torch.autograd.grad(val, [vb], tg, retain_graph=True)
    R.check_grad(ga.cpu().numpy(), gA, l1A, 'f64', 'dyadic', '%s gA alone' % path)
    R.check_grad(gb.cpu().numpy(), gB, l1B, 'f64', 'dyadic', '%s gB alone' % path)
    # value-less B: gA as if B were all ones; value-less A: gB likewise
    gA1, _, l1A1, _ = R.oracle(case, va64, None, g64)
    _, gB1, _, l1B1 = R.oracle(case, None, vb64, g64)
    va = _leaf(va64, None, 'f64', dev)
    run(va, None)[2].backward(tg)
    R.check_grad(_grad_np(va, None), gA1, l1A1, 'f64', 'dyadic', '%s value-less B' % path)
    vb = _leaf(vb64, None, 'f64', dev)
    run(None, vb)[2].backward(tg)
    R.check_grad(_grad_np(vb, None), gB1, l1B1, 'f64', 'dyadic', '%s value-less A' % path)


def test_scripted_spspmm_carries_the_same_gradients(dev):
    case = public_case('random')
    va64, vb64, g64 = R.values(case, 'uniform', 4)
    jit = torch.jit.script(spspmm_tensor)
    grads = []
    for fn in (jit, spspmm_tensor):
        va, vb = _leaf(va64, None, 'f32', dev), _leaf(vb64, None, 'f32', dev)
        A = SparseTensor(rowptr=t(case['rowptrA'], dev), col=t(case['colA'], dev), value=va,
                         sparse_sizes=(case['m'], case['k']), is_sorted=True, trust_data=True)
        B = SparseTensor(rowptr=t(case['rowptrB'], dev), col=t(case['colB'], dev), value=vb,
                         sparse_sizes=(case['k'], case['N']), is_sorted=True, trust_data=True)
        C = fn(A, B, 'sum')
        C.storage.value().backward(t(R.stored(g64, 'f32'), dev))
        grads.append((_grad_np(va, None), _grad_np(vb, None)))
    assert np.array_equal(grads[0][0].view(np.uint8), grads[1][0].view(np.uint8))
    assert np.array_equal(grads[0][1].view(np.uint8), grads[1][1].view(np.uint8))
    f32 = lambda a: R.stored(a, 'f32').astype(np.float64)  # noqa: E731
    gA, gB, l1A, l1B = R.oracle(case, f32(va64), f32(vb64), f32(g64))
    R.check_grad(grads[0][0], gA, l1A, 'f32', 'uniform', 'scripted gA')
    R.check_grad(grads[0][1], gB, l1B, 'f32', 'uniform', 'scripted gB')


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_no_grad_path_is_todays(dev, dtype):
    case = public_case('random')
    va64, vb64, _ = R.values(case, 'uniform', 6)
    ops = [t(case[k], dev) for k in ('rowptrA', 'colA', 'rowptrB', 'colB')]
    va, vb = _leaf(va64, None, dtype, dev, False), _leaf(vb64, None, dtype, dev, False)
    bare = torch.ops.tsamd.spspmm(ops[0], ops[1], va, ops[2], ops[3], vb, case['N'], True)  # positional, 8 arguments
    assert bare[2].grad_fn is None

    def same(out):
        return all(torch.equal(a, b) for a, b in zip(out[:2], bare[:2])) and \
            np.array_equal(out[2].detach().cpu().numpy().view(np.uint8), bare[2].cpu().numpy().view(np.uint8))

    run, _, _ = make_path('tensor', case, dev)
    out = run(va, vb)
    assert out[2].grad_fn is None and not out[2].requires_grad and same(out)
    vag, vbg = va.clone().requires_grad_(True), vb.clone().requires_grad_(True)
    with torch.no_grad():
        out = run(vag, vbg)
        idx, val = spspmm_functional(t(np.stack([case['rowA'], case['colA']]), dev), vag,
                                     t(np.stack([case['rowB'], case['colB']]), dev), vbg, case['m'], case['k'], case['N'])
    assert out[2].grad_fn is None and not out[2].requires_grad and same(out)
    assert val.grad_fn is None and torch.equal(val, bare[2]) and torch.equal(idx[1], bare[1])
    # with a graph the forward values are the same bits too
    out = run(vag, vbg)
    assert out[2].grad_fn is not None and same(out)
    assert matmul(SparseTensor(rowptr=ops[0], col=ops[1], sparse_sizes=(case['m'], case['k']), is_sorted=True, trust_data=True),
                  SparseTensor(rowptr=ops[2], col=ops[3], sparse_sizes=(case['k'], case['N']), is_sorted=True,
                               trust_data=True)).storage.value() is None
