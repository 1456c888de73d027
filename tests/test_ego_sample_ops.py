"""torch_sparse::ego_k_hop_sample_adj (ShaDow-GNN's sampler) is registered with the reference's schema
(csrc/ego_sample.cpp, the schema RegisterOperators infers) and compiles inside TorchScript.  No GPU needed."""
import pytest
import torch

import pytorch_sparse_amd  # noqa: F401

SCHEMA = ('torch_sparse::ego_k_hop_sample_adj(Tensor _0, Tensor _1, Tensor _2, int _3, int _4, bool _5) -> '
          '(Tensor _0, Tensor _1, Tensor _2, Tensor _3, Tensor _4, Tensor _5)')


def test_ego_k_hop_sample_adj_schema():
    assert str(torch.ops.torch_sparse.ego_k_hop_sample_adj.default._schema) == SCHEMA


def test_ego_k_hop_sample_adj_scripts():
    @torch.jit.script
    def ego(rowptr: torch.Tensor, col: torch.Tensor, idx: torch.Tensor, depth: int, k: int):
        rp, c, n_id, e_id, ptr, root = torch.ops.torch_sparse.ego_k_hop_sample_adj(rowptr, col, idx, depth, k, False)
        return rp, c, n_id, e_id, ptr, root

    assert 'ego_k_hop_sample_adj' in str(ego.graph)


def test_ego_k_hop_sample_adj_refuses_cpu_tensors():
    rowptr, col = torch.tensor([0, 1, 2]), torch.tensor([1, 0])
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        torch.ops.torch_sparse.ego_k_hop_sample_adj(rowptr, col, torch.tensor([0]), 1, 2, False)
