"""Timings of SparseTensor.matmul_rel (csrc/rel_gemm.hip) against the loop a relational layer writes today,

    loop   sum over r of  adj.masked_select_nnz(rel == r).matmul(x @ W[r])            (x @ W[r] in rocBLAS)
    rel    adj.matmul_rel(x, W, rel)

forward and forward + backward w.r.t. x and W, both sides timed in this process on this device, alternating: HIP-event
medians of --repeat calls after --warmup, the kernels one call launches (torch.profiler) and the peak memory of one
call.  Graphs rmat_scale20_ef20 and uniform_deg20_2^21, R in 4, 16, 64 with the relations drawn uniformly and with a
skewed law (P(r) ~ 1 / (r + 1)), F = Fo in 64, 128, fp32 and bf16.  Appends one JSON line per case to --out; --table
prints the README table of a results file.

    python scripts/bench_matmul_rel.py [--repeat 20] [--warmup 3] [--small] [--out profiles/matmul_rel_bench.jsonl]
    python scripts/bench_matmul_rel.py --table profiles/matmul_rel_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_attention import launches  # noqa: E402
from bench_fused_attention import peak_mib  # noqa: E402

LEGS = (('fw', 'forward'), ('fwbw', 'forward + backward'))


def timed_pair(a, b, repeat, warmup):
    """HIP-event medians of `repeat` calls of a and of b, one call of each in turn, after `warmup` of both"""
    ms = ([], [])
    for i in range(warmup + repeat):
        for side, fn in enumerate((a, b)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if i >= warmup:
                ms[side].append(t0.elapsed_time(t1))
    return [round(sorted(m)[len(m) // 2], 4) for m in ms]


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['graph', 'R', 'law', 'F = Fo', 'dtype', 'pairs']
    for _, leg in LEGS:
        head += ['%s: loop' % leg, 'matmul_rel']
    head += ['launches: loop -> rel', 'peak MiB: loop -> rel']
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        cells = [r['graph'], str(r['R']), r['law'], str(r['F']), r['dtype'], str(r['pairs'])]
        for k, _ in LEGS:
            ours, theirs = r[k + '_ms'], r[k + '_ms_loop']
            cells += ['%.3g ms' % theirs, '%.3g ms%s' % (ours, ' (slower)' if ours > theirs else '')]
        cells.append(', '.join('%s -> %s' % (r[k + '_launches_loop'], r[k + '_launches']) for k, _ in LEGS))
        cells.append(', '.join('%.0f -> %.0f' % (r[k + '_peak_mib_loop'], r[k + '_peak_mib']) for k, _ in LEGS))
        print('| ' + ' | '.join(cells) + ' |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1', help='which of the two graphs to run')
    ap.add_argument('--relations', default='4,16,64')
    ap.add_argument('--widths', default='64,128')
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matmul_rel_bench.jsonl'))
    ap.add_argument('--table', metavar='JSONL', help='print the README table of a results file and exit')
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import pytorch_sparse_amd as ts
    from pytorch_sparse_amd import synth
    assert torch.cuda.is_available(), 'the benchmark needs the GPU'
    dev = torch.device('cuda:0')
    rmat, uni = (14, 14) if args.small else (20, 21)
    graphs = [('rmat_scale%d_ef20' % rmat, lambda: synth.rmat_csr(rmat, 20, seed=0, device=dev)),
              ('uniform_deg20_2^%d' % uni, lambda: synth.uniform_degree_csr(1 << uni, 1 << uni, 20, device=dev))]
    for name, make in [graphs[int(i)] for i in args.graphs.split(',')]:
        rowptr, col = make()
        n, E = rowptr.numel() - 1, int(col.numel())
        adj = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
        adj.storage.row(), adj.storage.colptr(), adj.storage.csr2csc()  # the caches of a training loop's second step
        for R in [int(r) for r in args.relations.split(',')]:
            for law in ('uniform', 'skewed'):
                g = torch.Generator(device=dev).manual_seed(R)
                p = torch.ones(R, device=dev) if law == 'uniform' else 1.0 / torch.arange(1, R + 1, device=dev)
                rel = torch.multinomial(p, E, replacement=True, generator=g)
                pairs = int(torch.unique(adj.storage.row() * R + rel).numel())
                for F in [int(f) for f in args.widths.split(',')]:
                    for dtype in [getattr(torch, d) for d in args.dtypes.split(',')]:
                        x = torch.randn((n, F), generator=g, device=dev).to(dtype).requires_grad_()
                        w = (torch.randn((R, F, F), generator=g, device=dev) / F ** 0.5).to(dtype).requires_grad_()
                        gout = torch.randn((n, F), generator=g, device=dev).to(dtype)

                        def loop():
                            out = None
                            for r in range(R):
                                y = adj.masked_select_nnz(rel == r, layout='coo').matmul(x @ w[r])
                                out = y if out is None else out + y
                            return out

                        def ours():
                            return adj.matmul_rel(x, w, rel)

                        rec = {'bench': 'matmul_rel', 'graph': name, 'n': n, 'entries': E, 'R': R, 'law': law, 'pairs': pairs,
                               'F': F, 'dtype': str(dtype).replace('torch.', ''), 'device': torch.cuda.get_device_name(0)}
                        legs = {'fw': (lambda: ours().detach(), lambda: loop().detach()),
                                'fwbw': (lambda: torch.autograd.grad(ours(), [x, w], gout),
                                         lambda: torch.autograd.grad(loop(), [x, w], gout))}
                        for leg, (a, b) in legs.items():
                            rec[leg + '_ms'], rec[leg + '_ms_loop'] = timed_pair(a, b, args.repeat, args.warmup)
                            rec[leg + '_launches_loop'], rec[leg + '_launches'] = launches(b), launches(a)
                            rec[leg + '_peak_mib_loop'], rec[leg + '_peak_mib'] = peak_mib(b), peak_mib(a)
                            torch.cuda.empty_cache()
                        print(json.dumps(rec), flush=True)
                        with open(args.out, 'a') as fh:
                            fh.write(json.dumps(rec) + '\n')
                        del x, w, gout, legs
                        torch.cuda.empty_cache()
                del rel
        del adj, rowptr, col
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
