"""Timings of SparseTensor.gat_attention (csrc/attention.hip, additive score mode) against the chain a GAT layer had to
write out before,

    chain   adj.set_value(leaky_relu(a_dst[row] + a_src[col], slope), 'coo').softmax(1).matmul_heads(v)
    fused   adj.gat_attention(a_dst, a_src, v, slope)

forward and forward + backward w.r.t. a_dst, a_src and v, both timed in this process on this device: HIP-event medians
of --repeat calls after --warmup, the kernels one call launches (torch.profiler) and torch.cuda.max_memory_allocated
over one call, above what was allocated before it.  Graphs are those of scripts/bench_fused_attention.py: the north-star
R-MAT scale 21, the R-MAT of BASELINE.json configs[2], a uniform degree-20 control, each at (H, D) = (1, 64), (8, 8),
(8, 16), (8, 64) in fp32 and bf16.  Appends one JSON line per (graph, H, D, dtype) to --out; --table prints the README
table of a results file.

    python scripts/bench_gat_attention.py [--repeat 20] [--warmup 3] [--small] [--out profiles/gat_attention_bench.jsonl]
    python scripts/bench_gat_attention.py --table profiles/gat_attention_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_attention import launches, timed  # noqa: E402
from bench_fused_attention import PAIRS, peak_mib, table  # noqa: E402

SLOPE = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1,2', help='which of the three graphs to run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gat_attention_bench.jsonl'))
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
        longest = int((rowptr[1:] - rowptr[:-1]).max())
        for H, D in ((1, 64), (8, 8), (8, 16), (8, 64)):
            for dtype in (torch.float32, torch.bfloat16):
                g = torch.Generator(device=dev).manual_seed(1)
                a_dst, a_src = (torch.randn((n, H), generator=g, device=dev).to(dtype) for _ in range(2))
                v = torch.randn((n, H, D), generator=g, device=dev).to(dtype)
                gout = torch.randn((n, H, D), generator=g, device=dev).to(dtype)

                def chain(a_dst=a_dst, a_src=a_src, v=v):
                    s = torch.nn.functional.leaky_relu(a_dst[row] + a_src[col], SLOPE)
                    return adj.set_value(s, layout='coo').softmax(1).matmul_heads(v)

                def fused(a_dst=a_dst, a_src=a_src, v=v):
                    return adj.gat_attention(a_dst, a_src, v, SLOPE)

                leaves = tuple(t.clone().requires_grad_() for t in (a_dst, a_src, v))
                calls = {
                    'fw': (fused, chain),
                    'fwbw': (lambda: torch.autograd.grad(fused(*leaves), leaves, gout),
                             lambda: torch.autograd.grad(chain(*leaves), leaves, gout)),
                }
                rec = {'bench': 'gat_attention', 'graph': name, 'n': n, 'entries': E, 'longest_row': longest, 'H': H,
                       'D': D, 'dtype': str(dtype).replace('torch.', ''), 'negative_slope': SLOPE,
                       'device': torch.cuda.get_device_name(0)}
                for key, (ours, theirs) in calls.items():
                    rec[key + '_ms_chain'] = timed(theirs, args.repeat, args.warmup)
                    rec[key + '_ms'] = timed(ours, args.repeat, args.warmup)
                    rec[key + '_speedup'] = round(rec[key + '_ms_chain'] / rec[key + '_ms'], 2)
                    rec[key + '_launches_chain'], rec[key + '_launches'] = launches(theirs), launches(ours)
                    rec[key + '_peak_mib_chain'], rec[key + '_peak_mib'] = peak_mib(theirs), peak_mib(ours)
                    torch.cuda.empty_cache()
                with torch.no_grad():
                    rec['max_abs_diff'] = float((fused().double() - chain().double()).abs().max())
                print(json.dumps(rec), flush=True)
                with open(args.out, 'a') as fh:
                    fh.write(json.dumps(rec) + '\n')
                del a_dst, a_src, v, gout, leaves, calls
                torch.cuda.empty_cache()
        del adj, rowptr, col, row
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
