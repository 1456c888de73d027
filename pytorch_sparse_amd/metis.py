"""Graph partitioning entry point (reference: torch_sparse/metis.py).  The reference copies the graph to the CPU and
hands it to METIS (csrc/cpu/metis_cpu.cpp), and raises "Not compiled with METIS support" in a build without that
library.  No METIS exists for this build: a SparseTensor on the GPU is partitioned there by the multilevel k-way
partitioner of csrc/partition.hip (docs/design/partition.md) behind the reference's three ops; one on the CPU with
`num_parts > 1` keeps raising the reference's error.  `recursive` is accepted and runs the same k-way scheme."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from .select import permute
from .tensor import SparseTensor


def weight2metis(weight: Tensor) -> Optional[Tensor]:
    """Float weights -> the integer weights the partitioner takes (torch_sparse/metis.py:10-21): None when all are
    equal, else (weight - min) / range scaled so that the smallest gap between two sorted weights maps to the numerator
    of its exact binary fraction, truncated to int64."""
    ordered = weight.sort()[0]
    gaps = ordered[1:] - ordered[:-1]
    if gaps.sum() == 0:
        return None
    low, span = ordered[0], ordered[-1] - ordered[0]
    numerator, denominator = (gaps.min() / span).item().as_integer_ratio()
    return (weight - low).div_(span).mul_(denominator).add_(numerator).to(torch.long)


def partition(src: SparseTensor, num_parts: int, recursive: bool = False, weighted: bool = False,
              node_weight: Optional[Tensor] = None, balance_edge: bool = False
              ) -> Tuple[SparseTensor, Tensor, Tensor]:
    assert num_parts >= 1
    if num_parts == 1:
        partptr = torch.tensor([0, src.size(0)], device=src.device())
        perm = torch.arange(src.size(0), device=src.device())
        return src, partptr, perm

    if balance_edge and node_weight is not None:
        raise ValueError("Cannot set 'balance_edge' and 'node_weight' at the same time in 'partition'")
    if not src.device().type == 'cuda':
        raise RuntimeError('Not compiled with METIS support')

    rowptr, col, value = src.csr()
    if value is not None and weighted:
        assert value.numel() == col.numel()
        value = value.view(-1).detach()
        if value.is_floating_point():
            value = weight2metis(value)
    else:
        value = None

    if balance_edge:
        node_weight = col.new_zeros(rowptr.numel() - 1)
        node_weight.scatter_add_(0, col, torch.ones_like(col))

    if node_weight is not None:
        assert node_weight.numel() == rowptr.numel() - 1
        node_weight = node_weight.view(-1).detach().to(col.device)
        if node_weight.is_floating_point():
            node_weight = weight2metis(node_weight)
        cluster = torch.ops.torch_sparse.partition2(rowptr, col, value, node_weight, num_parts, recursive)
    else:
        cluster = torch.ops.torch_sparse.partition(rowptr, col, value, num_parts, recursive)

    cluster, perm = cluster.sort(stable=True)
    out = permute(src, perm)
    partptr = torch.ops.torch_sparse.ind2ptr(cluster, num_parts)
    return out, partptr, perm


SparseTensor.partition = partition
