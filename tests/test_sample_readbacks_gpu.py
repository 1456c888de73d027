"""What a change of the sampler glue (csrc/ops_sample*.cpp, csrc/ops_sample.h) must not move, for the operators whose
suites do not pin it: the number of host read-backs of one call, and how far a call advances torch's CPU generator.
(hetero_neighbor_sample, hetero_temporal_neighbor_sample and hgt_sample have their counts in their own suites.)

The graph: 64 nodes, the degrees 0, 1, k-1, k, k+1 for k = 3 in turn; 8 seeds, one of them listed twice; 2 hops /
depth 2.  Every expected count was measured on the glue before its shared steps moved into ops_sample.h and is
asserted as an equality: one more is a new stall per mini-batch, one fewer means a size is no longer read."""
import pytest
import torch

import pytorch_sparse_amd  # noqa: F401  (registers the torch_sparse:: ops)
from tests.util import _count_syncs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ops = torch.ops.torch_sparse
K = 3
N = 64


@pytest.fixture(scope='module')
def graph():
    g = torch.Generator().manual_seed(0)
    deg = torch.tensor([0, 1, K - 1, K, K + 1]).repeat(13)[:N]
    rowptr = torch.zeros(N + 1, dtype=torch.long)
    rowptr[1:] = deg.cumsum(0)
    col = torch.randint(0, N, (int(rowptr[-1]), ), generator=g)
    seeds = torch.tensor([0, 1, 2, 3, 4, 13, 22, 3])  # every degree, node 3 twice
    assert set(deg[seeds].tolist()) == {0, 1, K - 1, K, K + 1}
    return rowptr.to(DEV), col.to(DEV), seeds.to(DEV)


def _calls(rowptr, col, seeds):
    return {
        'sample_adj_draw': lambda: ops.sample_adj(rowptr, col, seeds, K, False),
        'sample_adj_take_all': lambda: ops.sample_adj(rowptr, col, seeds, -1, False),
        'neighbor_sample_directed': lambda: ops.neighbor_sample(rowptr, col, seeds, [K, K], False, True),
        'neighbor_sample_undirected': lambda: ops.neighbor_sample(rowptr, col, seeds, [K, K], False, False),
        'relabel_one_hop': lambda: ops.relabel_one_hop(rowptr, col, None, seeds, False),
        'saint_subgraph': lambda: ops.saint_subgraph(seeds, rowptr, torch.empty(0, dtype=torch.long, device=DEV), col),
        'ego_k_hop_sample_adj': lambda: ops.ego_k_hop_sample_adj(rowptr, col, seeds, 2, K, False),
    }


READ_BACKS = {
    # sample_adj: "Two host syncs" -- the size of the draw, the relabel's number of new nodes
    'sample_adj_draw': 2,
    'sample_adj_take_all': 2,
    # neighbor_sample: "Two host read-backs per hop" (size of the draw; length of the node list), 2 hops
    'neighbor_sample_directed': 4,
    # ... + induced_entries_bipartite's "Two host syncs" for the edges between the sampled nodes
    'neighbor_sample_undirected': 6,
    # relabel_one_hop: "sync 1" of select_segments, "sync 2" of the relabel
    'relabel_one_hop': 2,
    # saint_subgraph: induced_entries_bipartite's "Two host syncs"
    'saint_subgraph': 2,
    # ego_k_hop_sample_adj: "one per hop + the number of distinct (seed, node) pairs + the number of candidate entries
    # V + the number of kept entries", depth 2
    'ego_k_hop_sample_adj': 5,
}


@pytest.mark.parametrize('name', sorted(READ_BACKS))
def test_host_read_backs(graph, name):
    call = _calls(*graph)[name]
    call()  # the first call loads the kernels
    _, probe = _count_syncs(lambda: torch.ones(3, device=DEV).sum().item())
    assert probe >= 1  # the counter sees a read-back
    out, n_sync = _count_syncs(call)
    print('read-backs of %s: %d' % (name, n_sync))
    assert sum(t.numel() for t in out if t is not None) > 0
    assert n_sync == READ_BACKS[name], n_sync


def _one_host_seed():
    # what host_seed() (csrc/ops_sample.h) draws from torch's CPU generator
    torch.randint(0, torch.iinfo(torch.int64).max, (1, ), dtype=torch.long)


@pytest.mark.parametrize('name,seeds_drawn', [('sample_adj_take_all', 0), ('sample_adj_draw', 1),
                                              ('neighbor_sample_directed', 1), ('neighbor_sample_undirected', 1)])
def test_cpu_generator_consumption(graph, name, seeds_drawn):
    """Callers see how far a sampler advances torch's CPU generator: taking every neighbour leaves it untouched, a draw
    advances it exactly as ONE host_seed() does, however many hops follow."""
    call = _calls(*graph)[name]
    torch.manual_seed(1234)
    before = torch.get_rng_state()
    call()
    after = torch.get_rng_state()
    torch.manual_seed(1234)
    for _ in range(seeds_drawn):
        _one_host_seed()
    assert torch.equal(after, torch.get_rng_state())
    assert torch.equal(after, before) == (seeds_drawn == 0)
