"""Timings of reverse_cuthill_mckee (docs/design/rcm.md): the public call against the route it replaces -- the whole
symmetric matrix copied to the host, scipy's serial ordering, the permutation copied back, permute on the device --
in the same process on the same device.  Graphs: symmetrised R-MATs of pytorch_sparse_amd.synth (16 draws per row), a
1024 x 1024 grid with shuffled ids (about 2000 narrow levels) and the launch-bound 3000-node uniform graph of the tests.
Both routes are called with is_symmetric=True (the inputs are symmetric; neither pays for the check) and must return
the same permutation.  Appends one JSON line per graph to --out: median wall milliseconds of --repeat calls after one
warm-up, and the route statistics of tsamd::rcm.

    python scripts/bench_rcm.py [--repeat 3] [--scales 18 20] [--small] [--sweep] [--out profiles/rcm_bench.jsonl]

--sweep times tsamd::rcm_tuned alone (device-built stable seeds, so no host step) over node capacities and level
budgets of the one-workgroup route: the runs behind the shipped limits."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytorch_sparse_amd as ts  # noqa: E402
from pytorch_sparse_amd import synth  # noqa: E402
from pytorch_sparse_amd.select import permute  # noqa: E402


def scipy_route(src):
    """reverse_cuthill_mckee as it stood before the HIP ordering (is_symmetric=True)."""
    import scipy.sparse as sp
    sp_src = src.to_scipy(layout='csr')
    perm = sp.csgraph.reverse_cuthill_mckee(sp_src, symmetric_mode=True).copy()
    perm = torch.from_numpy(perm).to(torch.long).to(src.device())
    return permute(src, perm), perm


def sym_csr(row, col, n):
    return synth.to_csr(torch.cat([row, col]), torch.cat([col, row]), n, n)


def rmat(scale, dev):
    row, col = synth.rmat_edges(scale, 16, seed=0, device=dev)
    return sym_csr(row, col, 1 << scale)


def grid(side, dev, seed=0):
    idx = torch.arange(side * side, device=dev).view(side, side)
    r = torch.cat([idx[:, :-1].reshape(-1), idx[:-1].reshape(-1)])
    c = torch.cat([idx[:, 1:].reshape(-1), idx[1:].reshape(-1)])
    p = torch.randperm(side * side, generator=torch.Generator().manual_seed(seed)).to(dev)
    return sym_csr(p[r], p[c], side * side)


def uniform(dev):
    key = np.unique(np.random.default_rng(12).integers(0, 3000 * 3000, 30_000))
    key = torch.from_numpy(key).to(dev)
    return sym_csr(torch.div(key, 3000, rounding_mode='floor'), key % 3000, 3000)


def timed(fn, repeat):
    times, out = [], None
    for _ in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    rest = sorted(times[1:])
    return out, round(rest[len(rest) // 2], 3), round(times[0], 3)


STATS = ('levels', 'components', 'big_levels', 'small_launches', 'host_syncs')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--scales', type=int, nargs='*', default=[18, 20])
    ap.add_argument('--small', action='store_true', help='scale-14 R-MAT and a 128 x 128 grid (a quick look)')
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rcm_bench.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    scales, side = ([14], 128) if args.small else (args.scales, 1024)
    graphs = [('rmat_scale%d_ef16_sym' % s, lambda s=s: rmat(s, dev)) for s in scales]
    graphs += [('grid_%dx%d_shuffled' % (side, side), lambda: grid(side, dev)), ('uniform_3000', lambda: uniform(dev))]
    limits = [int(x) for x in torch.ops.tsamd.rcm_limits()]
    for name, make in graphs:
        rowptr, col = make()
        n = rowptr.numel() - 1
        adj = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
        base = {'bench': 'rcm', 'graph': name, 'n': n, 'entries': int(col.numel()), 'limits': limits,
                'device': torch.cuda.get_device_name(0)}
        deg = torch.ops.tsamd.rcm_degree(rowptr, col)
        ids = torch.arange(n, device=dev)
        stable = torch.ops.tsamd.sort_coo(deg, ids, int(col.numel()) + 2, n, True)[1]
        if args.sweep:
            for cap in (0, 64, 256, 1024):
                for budget in (64, 256, 1024, 4096):
                    if cap == 0 and budget != 256:
                        continue
                    (perm, stats), ms, _ = timed(lambda: torch.ops.tsamd.rcm_tuned(rowptr, col, stable, cap, budget),
                                                 args.repeat)
                    rec = dict(base, sweep=True, small_cap=cap, budget=budget, ms=ms, **dict(zip(STATS, stats.tolist())))
                    print(json.dumps(rec), flush=True)
                    with open(args.out, 'a') as fh:
                        fh.write(json.dumps(rec) + '\n')
            continue
        (_, perm), ms, first = timed(lambda: ts.reverse_cuthill_mckee(adj, True), args.repeat)
        (_, perm_stable), ms_stable, _ = timed(lambda: ts.reverse_cuthill_mckee(adj, True, seeds='stable'), args.repeat)
        (_, want), ms_scipy, _ = timed(lambda: scipy_route(adj), args.repeat)
        _, ms_order, _ = timed(lambda: torch.ops.tsamd.rcm(rowptr, col, stable, -1), args.repeat)
        _, stats = torch.ops.tsamd.rcm(rowptr, col, stable, -1)
        rec = dict(base, ms=ms, ms_first_call=first, ms_seeds_stable=ms_stable, ms_scipy_route=ms_scipy,
                   ms_ordering_only=ms_order, speedup=round(ms_scipy / ms, 2), same_perm=bool(torch.equal(perm, want)),
                   **dict(zip(STATS, stats.tolist())))
        print(json.dumps(rec), flush=True)
        with open(args.out, 'a') as fh:
            fh.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
