"""Timings of SparseTensor.gatv2_attention (csrc/gatv2.hip) against the chain a GATv2 layer writes out today,

    chain   z = x_src[col] + x_dst[row]; s = (leaky_relu(z, slope) * att).sum(-1)
            adj.set_value(s, 'coo').softmax(1).matmul_heads(x_src)
    fused   adj.gatv2_attention(x_dst, x_src, att, slope)

forward and forward + backward w.r.t. x_dst, x_src and att, both timed in this process on this device, one call of each
in turn: HIP-event medians of --repeat calls after --warmup, the kernels one call launches (torch.profiler) and
torch.cuda.max_memory_allocated over one call, above what was allocated before it.  Graphs and (H, D) cells are those of
scripts/bench_gat_attention.py.  A cell whose [nnz, H, D] tensor of the chain (with its backward copies: four of them)
does not fit in the free memory is skipped and named.  Every case passes a parity gate (fused against chain, float32)
before it is timed.  Appends one JSON line per (graph, H, D, dtype) to --out; --table prints the README table.

    python scripts/bench_gatv2_attention.py [--repeat 20] [--warmup 3] [--small] [--out profiles/gatv2_attention_bench.jsonl]
    python scripts/bench_gatv2_attention.py --table profiles/gatv2_attention_bench.jsonl"""
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

SLOPE = 0.2


def table(path):
    print('| graph | H x D | dtype | fw chain ms | fw fused ms | fw x | fw+bw chain ms | fw+bw fused ms | fw+bw x | '
          'peak MiB fw+bw chain / fused | launches fw+bw chain / fused |')
    print('|---|---|---|---|---|---|---|---|---|---|---|')
    for line in open(path):
        r = json.loads(line)
        if r.get('skipped'):
            print('| %s | %d x %d | %s | skipped: %s |' % (r['graph'], r['H'], r['D'], r['dtype'], r['skipped']))
            continue
        mark = lambda x: '%.2f%s' % (x, ' (slower)' if x < 1.0 else '')  # noqa: E731
        print('| %s | %d x %d | %s | %.3f | %.3f | %s | %.3f | %.3f | %s | %.0f / %.0f | %d / %d |' % (
            r['graph'], r['H'], r['D'], r['dtype'], r['fw_ms_chain'], r['fw_ms'], mark(r['fw_speedup']),
            r['fwbw_ms_chain'], r['fwbw_ms'], mark(r['fwbw_speedup']), r['fwbw_peak_mib_chain'], r['fwbw_peak_mib'],
            r['fwbw_launches_chain'], r['fwbw_launches']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1,2', help='which of the three graphs to run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gatv2_attention_bench.jsonl'))
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
        row = adj.storage.row()
        adj.storage.colptr(), adj.storage.csr2csc()  # the caches of a training loop's second step
        for H, D in ((1, 64), (8, 8), (8, 16), (8, 64)):
            for dtype in (torch.float32, torch.bfloat16):
                rec = {'bench': 'gatv2_attention', 'graph': name, 'n': n, 'entries': E, 'H': H, 'D': D,
                       'dtype': str(dtype).replace('torch.', ''), 'negative_slope': SLOPE,
                       'device': torch.cuda.get_device_name(0)}
                need = 4 * E * H * D * torch.empty((), dtype=dtype).element_size()
                free = torch.cuda.mem_get_info(dev)[0]
                if need > free:
                    rec['skipped'] = 'the chain needs %.1f GiB for its [nnz, H, D] tensors, %.1f GiB are free' % (
                        need / 2 ** 30, free / 2 ** 30)
                else:
                    g = torch.Generator(device=dev).manual_seed(1)
                    x_dst, x_src, gout = (torch.randn((n, H, D), generator=g, device=dev).to(dtype) for _ in range(3))
                    att = (torch.randn((H, D), generator=g, device=dev) / D ** 0.5).to(dtype)

                    def chain(x_dst=x_dst, x_src=x_src, att=att):
                        s = (torch.nn.functional.leaky_relu(x_src[col] + x_dst[row], SLOPE) * att).sum(-1)
                        return adj.set_value(s, layout='coo').softmax(1).matmul_heads(x_src)

                    def fused(x_dst=x_dst, x_src=x_src, att=att):
                        return adj.gatv2_attention(x_dst, x_src, att, SLOPE)

                    with torch.no_grad():  # the parity gate, on float32 copies of the same values
                        f32 = [t.float() for t in (x_dst, x_src, att)]
                        rec['max_abs_diff'] = float((fused(*f32) - chain(*f32)).abs().max())
                        assert rec['max_abs_diff'] < 1e-3, rec
                        del f32
                    leaves = tuple(t.clone().requires_grad_() for t in (x_dst, x_src, att))
                    calls = {'fw': (fused, chain),
                             'fwbw': (lambda: torch.autograd.grad(fused(*leaves), leaves, gout),
                                      lambda: torch.autograd.grad(chain(*leaves), leaves, gout))}
                    for key, (ours, theirs) in calls.items():
                        rec[key + '_ms_chain'] = timed(theirs, args.repeat, args.warmup)
                        rec[key + '_ms'] = timed(ours, args.repeat, args.warmup)
                        rec[key + '_speedup'] = round(rec[key + '_ms_chain'] / rec[key + '_ms'], 2)
                        rec[key + '_launches_chain'], rec[key + '_launches'] = launches(theirs), launches(ours)
                        rec[key + '_peak_mib_chain'], rec[key + '_peak_mib'] = peak_mib(theirs), peak_mib(ours)
                        torch.cuda.empty_cache()
                    del x_dst, x_src, att, gout, leaves, calls
                print(json.dumps(rec), flush=True)
                with open(args.out, 'a') as fh:
                    fh.write(json.dumps(rec) + '\n')
                torch.cuda.empty_cache()
        del adj, rowptr, col, row
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
