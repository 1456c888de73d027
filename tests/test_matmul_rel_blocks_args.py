"""SparseTensor.matmul_rel with a block-diagonal weight [R, B, ci, co]: the refusals that raise before any device call
(no GPU needed), and the TorchScript compilation of a module that passes one."""
import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import SparseTensor


def adj(value=None):
    return SparseTensor(rowptr=torch.tensor([0, 2, 3]), col=torch.tensor([0, 1, 1]), value=value, sparse_sizes=(2, 2),
                        is_sorted=True, trust_data=True)


X, W, REL = torch.ones(2, 4), torch.ones(3, 2, 2, 5), torch.tensor([0, 2, 1])
BAD = {
    'float16': dict(x=X.half(), weight=W.half()),
    'float64': dict(x=X.double(), weight=W.double()),
    'batched x': dict(x=X[None]),
    'value grad': dict(value=torch.ones(3, requires_grad=True)),
    'wide Fo': dict(weight=torch.ones(3, 2, 2, 257)),
    'wide F': dict(x=torch.ones(2, 514), weight=torch.ones(3, 2, 257, 5)),
    'dtype mismatch': dict(weight=W.bfloat16()),
    'B ci != F': dict(weight=torch.ones(3, 2, 3, 5)),
    'no block': dict(x=torch.ones(2, 0), weight=torch.ones(3, 0, 2, 5)),
    'empty block': dict(weight=torch.ones(3, 2, 2, 0)),
    'weight rank': dict(weight=W[None]),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_refused(case):
    kw = dict(x=X, weight=W, rel=REL, reduce='sum', value=None)
    kw.update(BAD[case])
    with pytest.raises(ValueError):
        adj(kw.pop('value')).matmul_rel(**kw)


def test_scripts():
    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.ones(3, 2, 2, 5))

        def forward(self, a: SparseTensor, x: torch.Tensor, rel: torch.Tensor) -> torch.Tensor:
            return ts.matmul_rel(a, x, self.weight, rel, 'mean')

    assert 'spmm_rel' in str(torch.jit.script(Layer()).inlined_graph)
