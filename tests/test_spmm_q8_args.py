"""SparseTensor.matmul_q8 / quantize_rows: the refusals that are decided before any device call, in Python and in the
C-ABI (fake pointers, never dereferenced), and the route query at a few literals.  No GPU needed."""
import ctypes

import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import SparseTensor, _native as nat

F32, F16, BF16, SUM, MEAN, MAX = 0, 2, 3, 0, 1, 3


def adj(value=None):
    return SparseTensor(rowptr=torch.tensor([0, 2, 3]), col=torch.tensor([0, 1, 1]), value=value, sparse_sizes=(2, 2),
                        is_sorted=True, trust_data=True)


def codes(*shape):
    return torch.zeros(shape).to(torch.float8_e4m3fn)


BAD = {
    'xq dtype': dict(xq=torch.zeros(2, 4)),
    'xq rank': dict(xq=codes(2, 4)[None]),
    'xq rows': dict(xq=codes(3, 4)),
    'wide F': dict(xq=codes(2, 1025)),
    'scale shape': dict(scale=torch.ones(3)),
    'scale rank': dict(scale=torch.ones(2, 1)),
    'scale dtype': dict(scale=torch.ones(2, dtype=torch.float64)),
    'values 2-D': dict(value=torch.ones(3, 2)),
    'value grad': dict(value=torch.ones(3, requires_grad=True)),
    'min': dict(reduce='min'),
    'max': dict(reduce='max'),
    'out dtype': dict(out_dtype=torch.float16),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_refused(case):
    kw = dict(xq=codes(2, 4), scale=None, reduce='sum', out_dtype=torch.float32, value=None)
    kw.update(BAD[case])
    with pytest.raises((ValueError, TypeError)):
        adj(kw.pop('value')).matmul_q8(**kw)


def test_cpu_tensors_and_other_dtypes_are_refused():
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ts.matmul_q8(adj(), codes(2, 4))
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ts.quantize_rows(torch.ones(2, 4))
    with pytest.raises(TypeError):
        ts.quantize_rows(torch.ones(2, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        ts.quantize_rows(torch.ones(4))


def test_status_codes():
    L, fake = nat.lib(), 0x1000
    big = 1 << 20

    def call(out_dtype=F32, reduce=SUM, rowptr=fake, col=fake, xq=fake, out=fake, M=4, N=4, F=16, E=4, ws=fake, nb=big):
        return L.tsamd_spmm_q8(out_dtype, reduce, rowptr, col, None, xq, None, out, M, N, F, E, ws, nb, None)

    assert call(M=-1) == 1 and call(E=-1) == 1
    assert call(reduce=MAX) == 2 and call(out_dtype=F16) == 2 and call(F=1025) == 2 and call(N=1 << 32) == 2
    assert call(M=0, rowptr=None, col=None, xq=None, out=None, ws=None, nb=0) == 0
    assert call(out=None) == 1 and call(rowptr=None) == 1 and call(col=None) == 1 and call(xq=None) == 1
    assert call(ws=None, nb=0) == 4 and call(nb=16) == 4 and call(ws=0x1008) == 4
    assert L.tsamd_quantize_rows(F32, fake, fake, fake, -1, 4, None) == 1
    assert L.tsamd_quantize_rows(1, fake, fake, fake, 4, 4, None) == 2  # float64
    assert L.tsamd_quantize_rows(F32, None, None, None, 0, 4, None) == 0
    assert L.tsamd_quantize_rows(F32, None, fake, fake, 4, 4, None) == 1


def test_workspace_and_route():
    L = nat.lib()
    assert L.tsamd_spmm_q8_workspace_bytes(F16, 10, 128, 1000) == 0
    assert L.tsamd_spmm_q8_workspace_bytes(F32, 10, 1025, 1000) == 0
    small, large = (L.tsamd_spmm_q8_workspace_bytes(BF16, 10, 128, E) for E in (1000, 100000))
    assert 0 < small < large
    words = (ctypes.c_int64 * 16)()
    # F -> (bytes per packet, lanes per row) for an aligned base; the chunk is 8 entries per lane of the group
    for F, want in {1: (1, 1), 16: (16, 1), 17: (1, 32), 24: (8, 4), 100: (4, 32), 128: (16, 8), 1024: (16, 64)}.items():
        assert L.tsamd_spmm_q8_route(F32, F, 100000, None, None, words) == 0
        assert (words[0], words[1]) == want and words[3] == 8 * words[1] and words[4] == 2048, F
        assert words[5] == -(-F // (words[0] * words[1])) and words[8] == -(-100000 // words[3])
        assert words[11] == 2 * words[9] + 2 * words[10] == L.tsamd_spmm_q8_workspace_bytes(F32, 10, F, 100000)
    # a base off the boundary narrows the packet, never the chunk (the workspace query cannot see it)
    assert L.tsamd_spmm_q8_route(F32, 128, 100000, 0x1004, None, words) == 0
    assert list(words[:6]) == [4, 8, 8, 64, 2048, 4]
    assert L.tsamd_spmm_q8_route(F32, 128, 100000, 0x1001, 0x1004, words) == 0
    assert list(words[:7]) == [1, 8, 8, 64, 2048, 16, 0]
    assert L.tsamd_spmm_q8_route(F32, 1025, 0, None, None, words) == 2 and L.tsamd_spmm_q8_route(F32, 8, 0, None, None, None) == 1
