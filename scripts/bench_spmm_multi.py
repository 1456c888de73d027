"""Timings of SparseTensor.matmul_multi (csrc/spmm_multi.hip) against the calls a multi-aggregation layer writes today,

    four   mean, min, max = (adj.matmul(x, r) for r in ...);  std = sqrt(relu(adj.matmul(x * x, 'mean') - mean ** 2))
    fused  adj.matmul_multi(x, ['mean', 'min', 'max', 'std'])
    two    adj.matmul(x, 'mean'), adj.matmul(x, 'max')      against      adj.matmul_multi(x, ['mean', 'max'])

forward and forward + backward w.r.t. x, both sides timed in this process on this device: HIP-event medians of --repeat
calls after --warmup, the kernels one call launches (torch.profiler) and the peak memory of one call.  Graphs are those
of scripts/bench_gat_attention.py, F in 32, 64, 128, fp32 and bf16.  Appends one JSON line per (graph, F, dtype) to
--out; --table prints the README table of a results file.

    python scripts/bench_spmm_multi.py [--repeat 20] [--warmup 3] [--small] [--out profiles/spmm_multi_bench.jsonl]
    python scripts/bench_spmm_multi.py --table profiles/spmm_multi_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_attention import launches, timed  # noqa: E402
from bench_fused_attention import peak_mib  # noqa: E402

CASES = (('four', 'mean, min, max, std'), ('two', 'mean, max'))
LEGS = (('fw', 'forward'), ('fwbw', 'forward + backward'))


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['graph', 'F', 'dtype']
    for _, what in CASES:
        for _, leg in LEGS:
            head += ['%s, %s: calls' % (what, leg), 'fused']
    head += ['launches: calls -> fused', 'peak MiB: calls -> fused']
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        cells = [r['graph'], str(r['F']), r['dtype']]
        keys = [c + '_' + k for c, _ in CASES for k, _ in LEGS]
        for key in keys:
            ours, theirs = r[key + '_ms'], r[key + '_ms_calls']
            cells += ['%.3g ms' % theirs, '%.3g ms%s' % (ours, ' (slower)' if ours > theirs else '')]
        cells.append(', '.join('%s -> %s' % (r[k + '_launches_calls'], r[k + '_launches']) for k in keys))
        cells.append(', '.join('%.0f -> %.0f' % (r[k + '_peak_mib_calls'], r[k + '_peak_mib']) for k in keys))
        print('| ' + ' | '.join(cells) + ' |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1,2', help='which of the three graphs to run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spmm_multi_bench.jsonl'))
    ap.add_argument('--table', metavar='JSONL', help='print the README table of a results file and exit')
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import pytorch_sparse_amd as ts
    from pytorch_sparse_amd import synth
    dev = torch.device('cuda:0')
    big, mid = (14, 13) if args.small else (21, 20)
    graphs = [('rmat_scale%d_ef20' % big, lambda: synth.rmat_csr(big, 20, seed=0, device=dev)),
              ('rmat_scale%d_ef20' % mid, lambda: synth.rmat_csr(mid, 20, seed=0, device=dev)),
              ('uniform_deg20_2^%d' % big, lambda: synth.uniform_degree_csr(1 << big, 1 << big, 20, device=dev))]
    for name, make in [graphs[int(i)] for i in args.graphs.split(',')]:
        rowptr, col = make()
        n, E = rowptr.numel() - 1, int(col.numel())
        adj = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
        adj.storage.row(), adj.storage.colptr(), adj.storage.csr2csc()  # the caches of a training loop's second step
        adj.storage.rowcount()
        for F in (32, 64, 128):
            for dtype in (torch.float32, torch.bfloat16):
                g = torch.Generator(device=dev).manual_seed(1)
                x = torch.randn((n, F), generator=g, device=dev).to(dtype)
                leaf = x.clone().requires_grad_()

                def four(x=x):
                    mean = adj.matmul(x, 'mean')
                    std = (adj.matmul(x * x, 'mean') - mean * mean).relu().sqrt()
                    return torch.stack([mean, adj.matmul(x, 'min'), adj.matmul(x, 'max'), std], 1)

                def two(x=x):
                    return torch.stack([adj.matmul(x, 'mean'), adj.matmul(x, 'max')], 1)

                sides = {'four': (lambda x=x: adj.matmul_multi(x, ['mean', 'min', 'max', 'std']), four),
                         'two': (lambda x=x: adj.matmul_multi(x, ['mean', 'max']), two)}
                rec = {'bench': 'spmm_multi', 'graph': name, 'n': n, 'entries': E, 'F': F,
                       'dtype': str(dtype).replace('torch.', ''), 'device': torch.cuda.get_device_name(0)}
                for case, (ours, theirs) in sides.items():
                    gout = torch.randn((n, 4 if case == 'four' else 2, F), generator=g, device=dev).to(dtype)
                    legs = {'fw': (ours, theirs),
                            'fwbw': (lambda f=ours, go=gout: torch.autograd.grad(f(leaf), leaf, go),
                                     lambda f=theirs, go=gout: torch.autograd.grad(f(leaf), leaf, go))}
                    for leg, (a, b) in legs.items():
                        key = case + '_' + leg
                        rec[key + '_ms_calls'] = timed(b, args.repeat, args.warmup)
                        rec[key + '_ms'] = timed(a, args.repeat, args.warmup)
                        rec[key + '_launches_calls'], rec[key + '_launches'] = launches(b), launches(a)
                        rec[key + '_peak_mib_calls'], rec[key + '_peak_mib'] = peak_mib(b), peak_mib(a)
                        torch.cuda.empty_cache()
                    del gout, legs
                print(json.dumps(rec), flush=True)
                with open(args.out, 'a') as fh:
                    fh.write(json.dumps(rec) + '\n')
                del x, leaf, sides
                torch.cuda.empty_cache()
        del adj, rowptr, col
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
