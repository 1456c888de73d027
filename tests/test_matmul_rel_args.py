"""SparseTensor.matmul_rel: the argument checks that raise before any device call (no GPU needed), and the TorchScript
compilation of a module that calls it."""
import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import SparseTensor


def adj(value=None):
    return SparseTensor(rowptr=torch.tensor([0, 2, 3]), col=torch.tensor([0, 1, 1]), value=value, sparse_sizes=(2, 2),
                        is_sorted=True, trust_data=True)


X, W, REL = torch.ones(2, 4), torch.ones(3, 4, 5), torch.tensor([0, 2, 1])
BAD = {
    'rel length': dict(rel=REL[:2]),
    'rel dtype': dict(rel=REL.int()),
    'dtype mismatch': dict(weight=W.bfloat16()),
    'float16': dict(x=X.half(), weight=W.half()),
    'float64': dict(x=X.double(), weight=W.double()),
    'weight rank': dict(weight=W[0]),
    'weight F': dict(weight=torch.ones(3, 5, 5)),
    'batched x': dict(x=X[None]),
    'x rows': dict(x=torch.ones(3, 4)),
    'wide Fo': dict(weight=torch.ones(3, 4, 513)),
    'reduce': dict(reduce='max'),
    'value grad': dict(value=torch.ones(3, requires_grad=True)),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_refused(case):
    kw = dict(x=X, weight=W, rel=REL, reduce='sum', value=None)
    kw.update(BAD[case])
    with pytest.raises(ValueError):
        adj(kw.pop('value')).matmul_rel(**kw)


def test_scripts():
    class Layer(torch.nn.Module):
        def forward(self, a: SparseTensor, x: torch.Tensor, w: torch.Tensor, rel: torch.Tensor) -> torch.Tensor:
            return ts.matmul_rel(a, x, w, rel, 'mean')

    assert 'spmm_rel' in str(torch.jit.script(Layer()).inlined_graph)
