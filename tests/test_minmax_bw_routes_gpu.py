"""Every row of the route table of the min / max backward (docs/design/spmm_backward.md), through the registered ops and
autograd: `torch.ops.torch_sparse.spmm_max` (the bare op: scatter) and `torch.ops.tsamd.spmm_minmax` (CSC arrays handed
over: one of the three pulls).  Which route ran is read off the op's second result -- [n, K] int64 ids, [n, K] int32 ids or
the 1-D int32 record buffer -- and off `storage.has_csr2csc()` for SparseTensor.matmul.  The pulls are deterministic:
their gradients equal those of the C-ABI entry called directly, bit for bit.  The scatter route is held to the bound of
tests/test_spmm_gpu.py::test_minmax_backward_route_rule."""
import functools

import pytest
import torch

from pytorch_sparse_amd import _native as nat
from pytorch_sparse_amd import synth
from tests.test_spmm_gpu import _csc_arrays, assert_within_scatter_bound
from tests.util import bits_equal

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graphs():
    """The `ragged` graph of tests/test_records_gpu.py cut down to 300 rows (few enough entries for the forward to keep
    records from K = 36 on: 32 bytes an entry against 12 bytes per output element) and its `tiny` graph."""
    g = torch.Generator().manual_seed(5)
    n = 300
    deg = torch.randint(0, 8, (n, ), generator=g)
    deg[::3] = 0            # empty rows
    deg[7] = 64             # exactly one step of the record writer
    deg[8] = 65
    deg[100] = 2500         # a row cut between many waves
    deg[n - 1] = 129
    rp = torch.zeros(n + 1, dtype=torch.int64)
    rp[1:] = deg.cumsum(0)
    c = torch.randint(0, n, (int(rp[-1]), ), generator=g)
    assert c.numel() * 32 <= 12 * n * 36
    out = [('ragged', rp, c, n) + _csc_arrays(rp, c, n)]
    rp, c = torch.tensor([0, 0, 3, 3, 4]), torch.tensor([1, 0, 3, 2])
    out.append(('tiny', rp, c, 4) + _csc_arrays(rp, c, 4))
    return out


def _second(arg, n, K):
    if arg.dim() == 1:
        assert arg.dtype == torch.int32
        return 'records'
    assert tuple(arg.shape) == (n, K)
    return {torch.int64: 'ids64', torch.int32: 'ids32'}[arg.dtype]


@pytest.mark.parametrize('dtype,K', [(torch.bfloat16, 36),   # 72-byte rows: no masked SDDMM, int32 ids are widened
                                     (torch.bfloat16, 64), (torch.bfloat16, 128), (torch.float32, 128),
                                     (torch.float64, 16)])  # fp64: the forward keeps no records
def test_every_route_through_the_ops(dev, dtype, K):
    import pytorch_sparse_amd as ts
    es = torch.empty(0, dtype=dtype).element_size()
    packets16 = (K * es) % 16 == 0
    for name, rp, c, n, colptr, perm, row in _graphs():
        d = lambda t: t.to(dev)  # noqa: E731
        x = synth.features(n, K, seed=2, dtype=dtype)
        if name == 'tiny':
            x[0, :3] = float('nan')  # a NaN beats nothing: elements without a winner
        v = synth.values(c.numel(), seed=3, dtype=dtype) - 0.3
        g = synth.features(n, K, seed=4, dtype=dtype)
        csr, csc = (d(rp), d(c)), (d(colptr), d(perm), d(row))
        arg64 = nat.spmm(*csr, d(v), d(x), 'max')[1]
        arg32 = nat.spmm_minmax_arg32(*csr, d(v), d(x), 'max')[1]
        assert torch.equal(arg64, arg32.long())
        for want_value in (False, True):
            tag = (name, want_value)
            # the C-ABI pull on ids, called directly; int32 ids give grad_value only as the masked SDDMM
            ids = arg32 if (not want_value or packets16) else arg64
            gv_ref, gm_ref = nat.spmm_minmax_bw_csc(*csr, d(v), d(x), d(g), ids, *csc, want_value=want_value, want_mat=True)
            gv_64, gm_64 = nat.spmm_minmax_bw_csc(*csr, d(v), d(x), d(g), arg64, *csc, want_value=want_value, want_mat=True)
            assert bits_equal(gm_ref, gm_64) and (not want_value or bits_equal(gv_ref, gv_64)), tag

            def run(op, want_mat=True):
                xr, vr = d(x).requires_grad_(want_mat), d(v).requires_grad_(want_value)
                out, second = op(xr, vr)
                out.backward(d(g))
                return _second(second, n, K), xr.grad, vr.grad

            def pull_equals_cabi(gx, gvv, what):
                assert bits_equal(gx, gm_ref), (tag, what)
                assert (gvv is None) == (not want_value), (tag, what)
                if want_value:
                    assert bits_equal(gvv, gv_ref), (tag, what)

            # the bare reference op: int64 ids, no CSC arrays -> scatter (atomics)
            kind, gx, gvv = run(lambda xr, vr: torch.ops.torch_sparse.spmm_max(*csr, vr, xr))
            assert kind == 'ids64' and gx is not None and (gvv is None) == (not want_value), tag
            assert_within_scatter_bound(c, v, x, g, arg64, gx, gvv, tag)
            # CSC arrays, winners returned as int64 ids -> pull on int64 ids
            kind, gx, gvv = run(lambda xr, vr: torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, True, False))
            assert kind == 'ids64', tag
            pull_equals_cabi(gx, gvv, 'ids64')
            # CSC arrays, winners kept by the node: records where the forward writes them and the backward can make
            # grad_value from them; int32 ids otherwise (widened in the backward when grad_value needs the row-parallel kernel)
            kind, gx, gvv = run(lambda xr, vr: torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, True, True))
            records = dtype != torch.float64 and (not want_value or packets16)
            assert kind == ('records' if records else 'ids32'), (tag, kind)
            pull_equals_cabi(gx, gvv, kind)
            # CSC arrays but no gradient w.r.t. mat: nothing to pull -> scatter, from int32 ids
            if want_value:
                kind, gx, gvv = run(lambda xr, vr: torch.ops.tsamd.spmm_minmax(*csr, vr, *csc, xr, True, True), want_mat=False)
                assert kind == 'ids32' and gx is None and gvv is not None, tag
                assert_within_scatter_bound(c, v, x, g, arg64, None, gvv, tag)
            # SparseTensor.matmul: the front-end's rule picks pull or scatter; has_csr2csc() says which
            xr, vr = d(x).requires_grad_(), d(v).requires_grad_(want_value)
            A = ts.SparseTensor(rowptr=csr[0], col=csr[1], value=vr, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
            A.matmul(xr, 'max').backward(d(g))
            if A.storage.has_csr2csc():
                pull_equals_cabi(xr.grad, vr.grad, 'matmul')
            else:
                assert xr.grad is not None and (vr.grad is None) == (not want_value), tag
                assert_within_scatter_bound(c, v, x, g, arg64, xr.grad, vr.grad, tag)
