"""Timings of SparseTensor.attention (csrc/attention.hip) against the three-step chain it fuses,

    chain   adj.sddmm(q, k, D ** -0.5).softmax(1).matmul_heads(v)
    fused   adj.attention(q, k, v)

forward and forward + backward w.r.t. q, k and v, both timed in this process on this device: HIP-event medians of
--repeat calls after --warmup, the kernels one call launches (torch.profiler) and torch.cuda.max_memory_allocated over
one call, above what was allocated before it.  Graphs and shapes are those of scripts/bench_attention.py: the north-star
R-MAT scale 21, the R-MAT of BASELINE.json configs[2], a uniform degree-20 control, each at (H, D) = (1, 64), (8, 16),
(8, 64) in fp32 and bf16.  Appends one JSON line per (graph, H, D, dtype) to --out; --table prints the README table of a
results file.

    python scripts/bench_fused_attention.py [--repeat 20] [--warmup 3] [--small] [--out profiles/fused_attention_bench.jsonl]
    python scripts/bench_fused_attention.py --table profiles/fused_attention_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_attention import launches, timed  # noqa: E402

PAIRS = (('fw', 'forward'), ('fwbw', 'forward + backward'))


def peak_mib(fn):
    """Device memory one call holds at its peak above what was allocated before it, MiB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return round((peak - base) / 2 ** 20, 1)


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['graph', 'H x D', 'dtype']
    for _, title in PAIRS:
        head += [title + ': chain', title + ': fused']
    head += ['launches (fw, fw + bw): chain -> fused', 'peak MiB (fw, fw + bw): chain -> fused']
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        cells = [r['graph'], '%d x %d' % (r['H'], r['D']), r['dtype']]
        for key, _ in PAIRS:
            ours, theirs = r[key + '_ms'], r[key + '_ms_chain']
            cells.append('%.3g ms' % theirs)
            cells.append('%.3g ms%s' % (ours, ' (slower)' if ours > theirs else ''))
        cells.append(', '.join('%s -> %s' % (r[key + '_launches_chain'], r[key + '_launches']) for key, _ in PAIRS))
        cells.append(', '.join('%.0f -> %.0f' % (r[key + '_peak_mib_chain'], r[key + '_peak_mib']) for key, _ in PAIRS))
        print('| ' + ' | '.join(cells) + ' |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1,2', help='which of the three graphs to run')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fused_attention_bench.jsonl'))
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
        longest = int((rowptr[1:] - rowptr[:-1]).max())
        for H, D in ((1, 64), (8, 16), (8, 64)):
            for dtype in (torch.float32, torch.bfloat16):
                g = torch.Generator(device=dev).manual_seed(1)
                q, k, v = (torch.randn((n, H, D), generator=g, device=dev).to(dtype) for _ in range(3))
                gout = torch.randn((n, H, D), generator=g, device=dev).to(dtype)
                scale = D ** -0.5

                def chain(q=q, k=k, v=v):
                    return adj.sddmm(q, k, scale).softmax(1).matmul_heads(v)

                def fused(q=q, k=k, v=v):
                    return adj.attention(q, k, v, scale)

                gq, gk, gv = (t.clone().requires_grad_() for t in (q, k, v))
                calls = {
                    'fw': (fused, chain),
                    'fwbw': (lambda: torch.autograd.grad(fused(gq, gk, gv), (gq, gk, gv), gout),
                             lambda: torch.autograd.grad(chain(gq, gk, gv), (gq, gk, gv), gout)),
                }
                rec = {'bench': 'fused_attention', 'graph': name, 'n': n, 'entries': E, 'longest_row': longest, 'H': H,
                       'D': D, 'dtype': str(dtype).replace('torch.', ''), 'device': torch.cuda.get_device_name(0)}
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
                del q, k, v, gout, gq, gk, gv, calls
                torch.cuda.empty_cache()
        del adj, rowptr, col
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
