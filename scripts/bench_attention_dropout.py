"""What dropout on the probabilities costs the fused attention calls (csrc/attention.hip, DROP instantiations), and what
it saves against the chain a layer with attention dropout had to write out before:

    chain    scores -> softmax(1) -> F.dropout on the [nnz, H] probabilities -> matmul_heads(v)
    fused    adj.gat_attention(a_dst, a_src, v, slope, dropout=0.6)   /   adj.attention(q, k, v, dropout=0.6)
    plain    the same fused call without dropout

forward and forward + backward w.r.t. the three operands, all timed in this process on this device: HIP-event medians of
--repeat calls after --warmup, and torch.cuda.max_memory_allocated over one call above what was allocated before it.
Graphs, shapes and dtypes are those of scripts/bench_gat_attention.py.  The fused call draws its seed from torch's CPU
generator on every call, as a training loop would.  Appends one JSON line per (mode, graph, H, D, dtype) to --out;
--table prints the README table of a results file.

    python scripts/bench_attention_dropout.py [--repeat 20] [--warmup 3] [--small] [--modes gat,dot]
    python scripts/bench_attention_dropout.py --table profiles/attention_dropout_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_attention import timed  # noqa: E402
from bench_fused_attention import peak_mib  # noqa: E402

SLOPE, RATE = 0.2, 0.6
KEYS = (('fw', 'forward'), ('fwbw', 'forward + backward'))


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['scores', 'graph', 'H x D', 'dtype']
    for _, title in KEYS:
        head += [title + ': chain with F.dropout', title + ': fused, no dropout', title + ': fused, dropout 0.6']
    head.append('peak MiB (fw, fw + bw): chain -> fused with dropout')
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        cells = [r['mode'], r['graph'], '%d x %d' % (r['H'], r['D']), r['dtype']]
        for key, _ in KEYS:
            ours, plain, theirs = r[key + '_ms'], r[key + '_ms_plain'], r[key + '_ms_chain']
            cells += ['%.3g ms' % theirs, '%.3g ms' % plain, '%.3g ms%s' % (ours, ' (slower)' if ours > theirs else '')]
        cells.append(', '.join('%.0f -> %.0f' % (r[key + '_peak_mib_chain'], r[key + '_peak_mib']) for key, _ in KEYS))
        print('| ' + ' | '.join(cells) + ' |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1,2', help='which of the three graphs to run')
    ap.add_argument('--modes', default='gat,dot', help='score modes: gat (additive), dot (dot product)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attention_dropout_bench.jsonl'))
    ap.add_argument('--table', metavar='JSONL', help='print the README table of a results file and exit')
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import pytorch_sparse_amd as ts
    from pytorch_sparse_amd import synth
    dropout = torch.nn.functional.dropout
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
        for mode in args.modes.split(','):
            for H, D in ((1, 64), (8, 8), (8, 16), (8, 64)):
                for dtype in (torch.float32, torch.bfloat16):
                    g = torch.Generator(device=dev).manual_seed(1)
                    score_shape = (n, H) if mode == 'gat' else (n, H, D)
                    sr, sc = (torch.randn(score_shape, generator=g, device=dev).to(dtype) for _ in range(2))
                    v = torch.randn((n, H, D), generator=g, device=dev).to(dtype)
                    gout = torch.randn((n, H, D), generator=g, device=dev).to(dtype)
                    if mode == 'gat':
                        def probabilities(sr, sc):
                            s = torch.nn.functional.leaky_relu(sr[row] + sc[col], SLOPE)
                            return adj.set_value(s, layout='coo').softmax(1)

                        def fused(sr=sr, sc=sc, v=v, rate=RATE):
                            return adj.gat_attention(sr, sc, v, SLOPE, dropout=rate)
                    else:
                        def probabilities(sr, sc):
                            return adj.sddmm(sr, sc, D ** -0.5).softmax(1)

                        def fused(sr=sr, sc=sc, v=v, rate=RATE):
                            return adj.attention(sr, sc, v, dropout=rate)

                    def chain(sr=sr, sc=sc, v=v):
                        p = probabilities(sr, sc)
                        return p.set_value(dropout(p.storage.value(), RATE, True), layout='coo').matmul_heads(v)

                    def plain(sr=sr, sc=sc, v=v):
                        return fused(sr, sc, v, 0.0)

                    leaves = tuple(t.clone().requires_grad_() for t in (sr, sc, v))
                    calls = {
                        'fw': (fused, plain, chain),
                        'fwbw': (lambda: torch.autograd.grad(fused(*leaves), leaves, gout),
                                 lambda: torch.autograd.grad(plain(*leaves), leaves, gout),
                                 lambda: torch.autograd.grad(chain(*leaves), leaves, gout)),
                    }
                    rec = {'bench': 'attention_dropout', 'mode': mode, 'graph': name, 'n': n, 'entries': E, 'H': H, 'D': D,
                           'dtype': str(dtype).replace('torch.', ''), 'dropout': RATE,
                           'device': torch.cuda.get_device_name(0)}
                    for key, (ours, bare, theirs) in calls.items():
                        rec[key + '_ms_chain'] = timed(theirs, args.repeat, args.warmup)
                        rec[key + '_ms_plain'] = timed(bare, args.repeat, args.warmup)
                        rec[key + '_ms'] = timed(ours, args.repeat, args.warmup)
                        rec[key + '_speedup'] = round(rec[key + '_ms_chain'] / rec[key + '_ms'], 2)
                        rec[key + '_dropout_cost'] = round(rec[key + '_ms'] / rec[key + '_ms_plain'], 3)
                        rec[key + '_peak_mib_chain'], rec[key + '_peak_mib'] = peak_mib(theirs), peak_mib(ours)
                        torch.cuda.empty_cache()
                    print(json.dumps(rec), flush=True)
                    with open(args.out, 'a') as fh:
                        fh.write(json.dumps(rec) + '\n')
                    del sr, sc, v, gout, leaves, calls
                    torch.cuda.empty_cache()
        del adj, rowptr, col, row
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
