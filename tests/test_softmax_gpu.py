"""csrc/softmax.hip against tests/softmax_reference.py: the two C entry points on every layout (route census asserted on
the host first), tsamd::segment_softmax, SparseTensor.softmax(dim) against the dense softmax, its gradient, and a
scripted module."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import softmax_reference as R
from tests.util import bits_equal, fromnp, tonp

pytestmark = pytest.mark.gpu

TORCH = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16, 'bf16': torch.bfloat16}
CASES = R.cases()
R.assert_reaches_every_route(CASES)  # hard: a layout that stops reaching a route fails the collection
GUARD = 64  # elements before and after the output that no call may touch


@pytest.fixture(scope='module')
def ts(dev):
    import pytorch_sparse_amd
    return pytorch_sparse_amd


def _call(backward, first, second, perm, ptr, nseg):
    """tsamd_segment_softmax / _bw through ctypes into the middle of a pre-filled buffer -> the output; the guard
    elements on either side must keep their bytes."""
    L = nat.lib()
    E = first.size(0)
    D = first.numel() // E if E else 3
    dt = nat.DTYPES[first.dtype]
    ws = nat.workspace(L.tsamd_segment_softmax_workspace_bytes(dt, nat._i64(E), nat._i64(D)), first.device)
    raw = torch.full(((E * D + 2 * GUARD) * first.element_size(), ), 85, dtype=torch.uint8, device=first.device)
    buf = raw.view(first.dtype)
    out = ctypes.c_void_p(buf.data_ptr() + GUARD * first.element_size())
    with torch.cuda.device(first.device):
        if backward:
            st = L.tsamd_segment_softmax_bw(dt, nat._ptr(first), nat._ptr(second), nat._ptr(perm), nat._ptr(ptr),
                                            nat._i64(nseg), nat._i64(E), nat._i64(D), out, nat._ptr(ws),
                                            ctypes.c_size_t(ws.numel()), nat.stream_ptr(first.device))
        else:
            st = L.tsamd_segment_softmax(dt, nat._ptr(first), nat._ptr(perm), nat._ptr(ptr), nat._i64(nseg),
                                         nat._i64(E), nat._i64(D), out, nat._ptr(ws), ctypes.c_size_t(ws.numel()),
                                         nat.stream_ptr(first.device))
    nat.check(st, 'tsamd_segment_softmax_bw' if backward else 'tsamd_segment_softmax')
    pad = GUARD * first.element_size()
    assert bool((raw[:pad] == 85).all()) and bool((raw[-pad:] == 85).all()), 'a byte outside [0, E * D) was written'
    return buf[GUARD:GUARD + E * D].view(first.shape).clone()


def _plan(dtype):
    """(layout, kind, D, random perm): fp32 takes every layout x kind; the other types every layout (so every route) with
    finite values, and every kind on the hub, the layout with all three routes and the long fold."""
    plan = []
    for case in CASES:
        for kind in R.KINDS:
            if dtype == 'f32' or kind in ('normal', 'late_max') or case.name == 'hub':
                plan.append((case, kind, 3, True))
        plan.append((case, 'normal', 1, False))
        plan.append((case, 'late_max', 3, False))
    return plan


@pytest.mark.parametrize('dtype', R.FLOATS)
def test_cabi_every_layout(dev, dtype):
    """Forward and backward: the comparators of the reference (bound, exact NaN / zero positions), the same bits from a
    second call, no byte outside the output written."""
    tdt = TORCH[dtype]
    rng = np.random.default_rng(7)
    worst_f = worst_b = 0.0
    for case, kind, D, shuffled in _plan(dtype):
        ptr = torch.from_numpy(case.ptr).to(dev)
        v = R.values(case, kind, dtype, D=D)
        g = R.grads(case, dtype, D=D)
        perm_np = rng.permutation(case.E) if shuffled else None
        if shuffled:
            for a in (v, g):
                a[perm_np] = a.copy()
        perm = None if perm_np is None else torch.from_numpy(perm_np).to(dev)
        value, grad = fromnp(v, tdt).to(dev), fromnp(g, tdt).to(dev)
        what = (case.name, kind, D, 'perm' if shuffled else 'plain')
        y = _call(False, value, None, perm, ptr, case.nseg)
        assert bits_equal(y, _call(False, value, None, perm, ptr, case.nseg)), ('forward not deterministic', ) + what
        gv = _call(True, y, grad, perm, ptr, case.nseg)
        assert bits_equal(gv, _call(True, y, grad, perm, ptr, case.nseg)), ('backward not deterministic', ) + what
        try:
            worst_f = max(worst_f, R.check_forward(tonp(y), v, perm_np, case.ptr, case.nseg, dtype))
            worst_b = max(worst_b, R.check_backward(tonp(gv), tonp(y), g, perm_np, case.ptr, case.nseg, dtype))
        except AssertionError as exc:
            raise AssertionError('%s: %s' % (what, exc)) from None
        if case.name == 'single' and kind in ('normal', 'late_max', 'big'):
            assert bool((y.double() == 1).all()), 'one segment of one entry is exactly 1'
    print('%s: worst err / bound forward %.3g backward %.3g' % (dtype, worst_f, worst_b))


def test_cabi_rejects_integers(dev):
    case = CASES[3]
    ptr = torch.from_numpy(case.ptr).to(dev)
    for tdt in (torch.int32, torch.int64, torch.uint8):
        value = torch.ones(case.E, dtype=tdt, device=dev)
        with pytest.raises(nat.TsamdError, match='tsamd_segment_softmax failed: unsupported dtype, reduction or size'):
            _call(False, value, None, None, ptr, case.nseg)


# ---- the public calls ------------------------------------------------------------------------------------------------
def _pattern():
    """300 x 200, rows 7..11 and columns 50..59 empty, row 123 a hub that holds every other column."""
    rng = np.random.default_rng(12)
    mask = rng.random((300, 200)) < 0.04
    mask[123] = True
    mask[7:12] = False
    mask[:, 50:60] = False
    row, col = np.nonzero(mask)
    return mask, row, col


@pytest.fixture(scope='module')
def pattern():
    return _pattern()


def _dense_softmax(mask, row, col, value, dim):
    """torch.softmax of the densified matrix with -inf at the absent positions, float64 -> the stored entries."""
    dense = torch.full(mask.shape + tuple(value.shape[1:]), -np.inf, dtype=torch.float64)
    dense[row, col] = value.double().cpu()
    return torch.softmax(dense, dim)[row, col]


@pytest.mark.parametrize('tdt', [torch.float64, torch.float32])
@pytest.mark.parametrize('heads', [0, 3])
def test_sparse_tensor_softmax_against_dense(ts, dev, pattern, tdt, heads):
    mask, row, col = pattern
    nnz = row.size
    shape = (nnz, heads) if heads else (nnz, )
    value = torch.from_numpy(np.random.default_rng(13).standard_normal(shape) * 4).to(tdt).to(dev)
    A = ts.SparseTensor(row=torch.from_numpy(row).to(dev), col=torch.from_numpy(col).to(dev), value=value,
                        sparse_sizes=mask.shape)
    caches = (A.storage.rowptr(), A.storage.colptr(), A.storage.csr2csc())
    rtol = 1e-12 if tdt == torch.float64 else 1e-5
    for dim in (1, 0, -1, -2) + ((2, ) if heads else ()):
        out = A.softmax(dim)
        assert isinstance(out, ts.SparseTensor) and out.sparse_sizes() == A.sparse_sizes()
        got = out.storage.value()
        assert got.shape == value.shape and got.dtype == tdt
        if dim == 2:
            want = torch.softmax(value.double().cpu(), 1)
        else:
            want = _dense_softmax(mask, row, col, value, dim % 2)
        assert bool(((got.double().cpu() - want).abs() <= rtol * want + 1e-300).all()), dim
        st = out.storage
        assert st.rowptr() is caches[0] and st.colptr() is caches[1] and st.csr2csc() is caches[2], 'caches are shared'
    assert bits_equal(ts.softmax(A, 1).storage.value(), A.softmax().storage.value())
    # the operator itself, on the column segments
    got = torch.ops.tsamd.segment_softmax(value, caches[2], caches[1], mask.shape[1])
    assert bits_equal(got, A.softmax(0).storage.value())


def test_sparse_tensor_softmax_without_value_and_with_integers(ts, dev, pattern):
    mask, row, col = pattern
    r, c = torch.from_numpy(row).to(dev), torch.from_numpy(col).to(dev)
    A = ts.SparseTensor(row=r, col=c, sparse_sizes=mask.shape)
    for dim, index, count in ((1, row, mask.sum(axis=1)), (0, col, mask.sum(axis=0))):
        got = A.softmax(dim).storage.value()
        assert got.dtype == torch.float32 and got.shape == (row.size, )
        want = torch.from_numpy(1.0 / count[index])
        assert bool(((got.double().cpu() - want).abs() <= 2.0 ** -23 * want).all())
    B = A.set_value(torch.ones(row.size, dtype=torch.int64, device=dev), layout='coo')
    for dim in (0, 1):
        with pytest.raises(ValueError):
            B.softmax(dim)
    with pytest.raises(IndexError):
        A.softmax(2)
    with pytest.raises(RuntimeError, match='float32, float64, float16 or bfloat16'):
        torch.ops.tsamd.segment_softmax(B.storage.value(), None, A.storage.rowptr(), mask.shape[0])
    E = ts.SparseTensor(row=r[:0], col=c[:0], value=torch.zeros(0, 3, device=dev), sparse_sizes=mask.shape)
    assert E.softmax(1).storage.value().shape == (0, 3) and E.softmax(0).storage.value().shape == (0, 3)


def test_softmax_then_matmul_gradients_against_dense(ts, dev, pattern):
    mask, row, col = pattern
    rng = np.random.default_rng(14)
    v = torch.from_numpy(rng.standard_normal(row.size) * 2).to(dev)
    x = torch.from_numpy(rng.standard_normal((200, 5))).to(dev)
    for dim in (1, 0):
        val, xx = v.clone().requires_grad_(), x.clone().requires_grad_()
        A = ts.SparseTensor(row=torch.from_numpy(row).to(dev), col=torch.from_numpy(col).to(dev), value=val,
                            sparse_sizes=mask.shape)
        (A.softmax(dim).matmul(xx) * xx.new_tensor([1., -2., 3., .5, 1.5])).sum().backward()
        dv, dx = v.cpu().clone().requires_grad_(), x.cpu().clone().requires_grad_()
        dense = torch.full(mask.shape, -np.inf, dtype=torch.float64)
        dense = dense.index_put((torch.from_numpy(row), torch.from_numpy(col)), dv)
        P = torch.softmax(dense, dim)
        P = torch.where(torch.from_numpy(mask), P, torch.zeros_like(P))  # empty rows / columns: NaN in the dense softmax
        ((P @ dx) * dx.new_tensor([1., -2., 3., .5, 1.5])).sum().backward()
        assert torch.allclose(val.grad.cpu(), dv.grad, rtol=1e-10, atol=1e-13), dim
        assert torch.allclose(xx.grad.cpu(), dx.grad, rtol=1e-10, atol=1e-13), dim


def test_gradcheck_of_segment_softmax_with_a_perm(ts, dev):
    from pytorch_sparse_amd.segment import segment_softmax
    rng = np.random.default_rng(15)
    ptr = torch.tensor([0, 0, 5, 6, 6, 23, 40], device=dev)
    perm = torch.from_numpy(rng.permutation(40)).to(dev)
    value = torch.from_numpy(rng.standard_normal((40, 2))).to(dev).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: segment_softmax(t, perm, ptr, 6), (value, ), nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda t: segment_softmax(t, None, ptr, 6), (value, ), nondet_tol=0.0)
    y = segment_softmax(value, perm, ptr, 6)
    g, = torch.autograd.grad((y * y).sum(), value, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):  # no second order
        g.sum().backward()


def test_scripted_module_calls_the_operator(ts, dev):
    class Attend(torch.nn.Module):
        def forward(self, score: torch.Tensor, rowptr: torch.Tensor, nseg: int) -> torch.Tensor:
            return torch.ops.tsamd.segment_softmax(score, None, rowptr, nseg)

    case = [c for c in CASES if c.name == 'boundaries'][0]
    ptr = torch.from_numpy(case.ptr).to(dev)
    value = torch.from_numpy(R.values(case, 'normal', 'f32')).to(dev)
    scripted = torch.jit.script(Attend())
    got = scripted(value, ptr, case.nseg)
    assert bits_equal(got, torch.ops.tsamd.segment_softmax(value, None, ptr, case.nseg))
    R.check_forward(tonp(got), tonp(value), None, case.ptr, case.nseg, 'f32')
