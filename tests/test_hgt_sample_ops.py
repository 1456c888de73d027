"""torch_sparse::hgt_sample (the operator behind PyG's HGTLoader) is registered with the reference's schema
(csrc/hgt_sample.cpp, the schema RegisterOperators infers), compiles inside TorchScript and refuses CPU tensors; and the
selection yardstick of the GPU tests (tests/hgt_reference.py: inclusion_probabilities) is pinned to the primitive the
reference draws with, torch.multinomial without replacement.  No GPU needed."""
from typing import Dict, List

import numpy as np
import pytest
import torch

import pytorch_sparse_amd  # noqa: F401
from tests.hgt_reference import LAW_BUDGETS, LAW_K, LAW_R, inclusion_probabilities, law_bound

SCHEMA = ('torch_sparse::hgt_sample(Dict(str, Tensor) _0, Dict(str, Tensor) _1, Dict(str, Tensor) _2, '
          'Dict(str, int[]) _3, int _4) -> (Dict(str, Tensor) _0, Dict(str, Tensor) _1, Dict(str, Tensor) _2, '
          'Dict(str, Tensor) _3)')


def test_hgt_sample_schema():
    assert str(torch.ops.torch_sparse.hgt_sample.default._schema) == SCHEMA


def test_hgt_sample_scripts():
    @torch.jit.script
    def hgt(colptr: Dict[str, torch.Tensor], row: Dict[str, torch.Tensor], inputs: Dict[str, torch.Tensor],
            num_samples: Dict[str, List[int]], num_hops: int):
        node, r, c, e = torch.ops.torch_sparse.hgt_sample(colptr, row, inputs, num_samples, num_hops)
        return node, r, c, e

    assert 'hgt_sample' in str(hgt.graph)


def test_hgt_sample_refuses_cpu_tensors():
    colptr = {'a__to__a': torch.tensor([0, 1, 2])}
    row = {'a__to__a': torch.tensor([1, 0])}
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        torch.ops.torch_sparse.hgt_sample(colptr, row, {'a': torch.tensor([0])}, {'a': [2]}, 1)


def test_the_law_vector_meets_the_normal_bound_conditions():
    pi = inclusion_probabilities(np.square(LAW_BUDGETS), LAW_K)
    assert abs(pi.sum() - LAW_K) < 1e-9
    assert (LAW_R * pi >= 50).all() and (LAW_R * (1 - pi) >= 50).all()


@pytest.mark.parametrize('gen_seed', [0, 1, 2])
def test_inclusion_probabilities_against_multinomial(gen_seed):
    """The yardstick against the reference's own primitive: R runs of torch.multinomial(budget ** 2, k, False) on the
    CPU, every candidate's count within the bound the GPU selection is held to."""
    w = np.square(np.asarray(LAW_BUDGETS, np.float64))
    pi = inclusion_probabilities(w, LAW_K)
    g = torch.Generator().manual_seed(gen_seed)
    wt = torch.tensor(w, dtype=torch.float32)
    count = np.zeros(len(w))
    for _ in range(LAW_R):
        count[torch.multinomial(wt, LAW_K, False, generator=g).numpy()] += 1
    dev = np.abs(count - LAW_R * pi) / law_bound(LAW_R, pi)
    print('largest deviation / bound: %.3f' % dev.max())
    assert (dev <= 1.0).all(), (count, LAW_R * pi)
