"""First timings of SparseTensor.partition (docs/design/partition.md): adj.partition(k) for k in {8, 1500} on a
1024 x 1024 grid with shuffled vertex ids and on the scale-20 R-MAT of pytorch_sparse_amd.synth (16 entries per row).
Appends one JSON line per (graph, k) to profiles/partition_bench.jsonl: the wall time of the whole call (median of
--repeat calls after one warm-up), the wall time of each phase from one extra call of tsamd::partition_timed (which
synchronises at the phase boundaries), the cut, the largest part and the capacity.

    python scripts/bench_partition.py [--repeat 3] [--small]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytorch_sparse_amd as ts  # noqa: E402
from pytorch_sparse_amd import synth  # noqa: E402


def grid_csr(h, w, dev, seed=0):
    idx = torch.arange(h * w, device=dev).view(h, w)
    r = torch.cat([idx[:, :-1].reshape(-1), idx[:-1].reshape(-1)])
    c = torch.cat([idx[:, 1:].reshape(-1), idx[1:].reshape(-1)])
    p = torch.randperm(h * w, generator=torch.Generator().manual_seed(seed)).to(dev)
    r, c = p[r], p[c]
    return synth.to_csr(torch.cat([r, c]), torch.cat([c, r]), h * w, h * w)


def cut_of(rowptr, col, cluster):
    """Entries of A + A^T (self-loops aside, duplicates merged) whose ends lie in different parts, every edge once."""
    n = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n, device=col.device), rowptr[1:] - rowptr[:-1])
    lo, hi = torch.minimum(row, col), torch.maximum(row, col)
    key = torch.unique(lo[lo != hi] * n + hi[lo != hi])
    return int((cluster[torch.div(key, n, rounding_mode='floor')] != cluster[key % n]).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='256 x 256 grid and scale-14 R-MAT (a quick look)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    side, scale = (256, 14) if args.small else (1024, 20)
    graphs = [('grid_%dx%d_shuffled' % (side, side), grid_csr(side, side, dev)),
              ('rmat_scale%d_ef16' % scale, synth.rmat_csr(scale, 16, seed=0, device=dev))]
    out = os.path.join(ROOT, 'profiles', 'partition_bench.jsonl')
    for name, (rowptr, col) in graphs:
        n = rowptr.numel() - 1
        adj = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
        for k in (8, 1500):
            times = []
            for i in range(args.repeat + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, partptr, perm = adj.partition(k)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            cluster, phase = torch.ops.tsamd.partition_timed(rowptr, col, None, None, k)
            sizes = partptr[1:] - partptr[:-1]
            rec = {'bench': 'partition', 'graph': name, 'n': n, 'entries': int(col.numel()), 'k': k,
                   'ms': round(sorted(times[1:])[len(times[1:]) // 2], 2), 'ms_first_call': round(times[0], 2),
                   'phase_ms': dict(zip(('level0', 'coarsen', 'initial', 'refine'), [round(x, 2) for x in phase])),
                   'cut': cut_of(rowptr, col, cluster), 'largest_part': int(sizes.max()),
                   'capacity': (103 * n) // (100 * k) + 1, 'device': torch.cuda.get_device_name(0)}
            print(json.dumps(rec), flush=True)
            with open(out, 'a') as fh:
                fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
