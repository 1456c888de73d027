"""The partition ops without a GPU: the reference's schemas (csrc/metis.cpp:18-69), the refusal of CPU tensors with the
reference's message, and weight2metis against outputs recorded from the reference's own function
(tests/golden/make_partition_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import metis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_schemas_equal_the_reference():
    with open(os.path.join(GOLDEN, 'partition_schemas.json')) as fh:
        want = json.load(fh)
    assert sorted(want) == ['mt_partition', 'partition', 'partition2']
    for name, schema in want.items():
        assert str(getattr(torch.ops.torch_sparse, name).default._schema) == schema, name


def test_phase_ops_are_registered():
    for name in ('partition_match', 'partition_contract', 'partition_initial', 'partition_refine'):
        assert hasattr(torch.ops.tsamd, name), name


def test_cpu_tensors_raise_the_metis_message():
    rowptr, col = torch.tensor([0, 1, 2]), torch.tensor([1, 0])
    nw = torch.ones(2, dtype=torch.long)
    with pytest.raises(RuntimeError, match='Not compiled with METIS support'):
        torch.ops.torch_sparse.partition(rowptr, col, None, 2, False)
    with pytest.raises(RuntimeError, match='Not compiled with METIS support'):
        torch.ops.torch_sparse.partition2(rowptr, col, None, nw, 2, True)
    with pytest.raises(RuntimeError, match='Not compiled with METIS support'):
        torch.ops.torch_sparse.mt_partition(rowptr, col, None, nw, 2, False, 4)
    A = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(2, 2), is_sorted=True)
    with pytest.raises(RuntimeError, match='Not compiled with METIS support'):
        A.partition(2)
    out, partptr, perm = A.partition(1)
    assert out is A and partptr.tolist() == [0, 2] and perm.tolist() == [0, 1]


def test_balance_edge_with_node_weight_raises():
    A = ts.SparseTensor(rowptr=torch.tensor([0, 1, 2]), col=torch.tensor([1, 0]), sparse_sizes=(2, 2), is_sorted=True)
    with pytest.raises(ValueError, match='balance_edge'):
        A.partition(2, node_weight=torch.ones(2), balance_edge=True)


def test_weight2metis_equals_the_reference():
    assert metis.weight2metis is ts.metis.weight2metis
    data = np.load(os.path.join(GOLDEN, 'partition_weight2metis.npz'))
    names = [k[3:] for k in data.files if k.startswith('in_')]
    assert len(names) >= 5 and any(int(data['none_' + n]) for n in names)
    for n in names:
        got = metis.weight2metis(torch.from_numpy(data['in_' + n].copy()))
        if int(data['none_' + n]):
            assert got is None, n
        else:
            assert got.dtype == torch.long and np.array_equal(got.numpy(), data['out_' + n]), n
