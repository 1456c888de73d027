"""Timings of SparseTensor.matmul_rel with a block-diagonal weight [R, B, ci, co] (csrc/rel_blocks.hip) against what
a layer writes without it,

    dense   adj.matmul_rel(x, dense(Q), rel)   dense(Q) the [R, F, Fo] weight scattered from Q with torch indexing on
                                               every call; in the backward autograd gathers the diagonal back out
    blocks  adj.matmul_rel(x, Q, rel)

forward and forward + backward w.r.t. x and Q, both sides timed in this process on this device, alternating: HIP-event
medians of --repeat calls after --warmup, the kernels one call launches (torch.profiler) and the peak memory of one
call.  Graph rmat_scale20_ef20, relations drawn uniformly, R in 16, 64, F = Fo in 64, 128, B in 2, 4, 8, 16, fp32 and
bf16.  Before a case is timed both sides must agree on the timed inputs: every element of out, grad_x and grad_Q
within 2 c u S (each side within c u S of the exact value; c of docs/design/widening.md, "Block-diagonal relational
SpMM", S from the same call on absolute values).  Appends one JSON line per case to --out; --table prints the README
table of a results file.

    python scripts/bench_matmul_rel_blocks.py [--repeat 20] [--warmup 3] [--small] [--out profiles/matmul_rel_blocks_bench.jsonl]
    python scripts/bench_matmul_rel_blocks.py --table profiles/matmul_rel_blocks_bench.jsonl"""
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
from bench_matmul_rel import LEGS, timed_pair  # noqa: E402

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}


def dense(q):
    """[R, B, ci, co] -> the block-diagonal [R, B ci, B co]"""
    R, B, ci, co = q.shape
    w = q.new_zeros((B, B, R, ci, co))
    idx = torch.arange(B, device=q.device)
    w[idx, idx] = q.transpose(0, 1)
    return w.permute(2, 0, 3, 1, 4).reshape(R, B * ci, B * co)


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['R', 'F = Fo', 'B', 'dtype', 'pairs']
    for _, leg in LEGS:
        head += ['%s: dense' % leg, 'blocks']
    head += ['launches: dense -> blocks', 'peak MiB: dense -> blocks']
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        cells = [str(r['R']), str(r['F']), str(r['B']), r['dtype'], str(r['pairs'])]
        for k, _ in LEGS:
            ours, theirs = r[k + '_ms'], r[k + '_ms_dense']
            cells += ['%.3g ms' % theirs, '%.3g ms%s' % (ours, ' (slower)' if ours > theirs else '')]
        cells.append(', '.join('%s -> %s' % (r[k + '_launches_dense'], r[k + '_launches']) for k, _ in LEGS))
        cells.append(', '.join('%.0f -> %.0f' % (r[k + '_peak_mib_dense'], r[k + '_peak_mib']) for k, _ in LEGS))
        print('| ' + ' | '.join(cells) + ' |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='a scale-14 graph (a quick look)')
    ap.add_argument('--relations', default='16,64')
    ap.add_argument('--widths', default='64,128')
    ap.add_argument('--blocks', default='2,4,8,16')
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'matmul_rel_blocks_bench.jsonl'))
    ap.add_argument('--table', metavar='JSONL', help='print the README table of a results file and exit')
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import pytorch_sparse_amd as ts
    from pytorch_sparse_amd import synth
    assert torch.cuda.is_available(), 'the benchmark needs the GPU'
    dev = torch.device('cuda:0')
    scale = 14 if args.small else 20
    name = 'rmat_scale%d_ef20' % scale
    rowptr, col = synth.rmat_csr(scale, 20, seed=0, device=dev)
    n, E = rowptr.numel() - 1, int(col.numel())
    adj = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
    row = adj.storage.row()
    adj.storage.colptr(), adj.storage.csr2csc()  # the caches of a training loop's second step
    d = int(torch.bincount(col, minlength=n).max())
    for R in [int(r) for r in args.relations.split(',')]:
        g = torch.Generator(device=dev).manual_seed(R)
        rel = torch.multinomial(torch.ones(R, device=dev), E, replacement=True, generator=g)
        pair, cnt = torch.unique(row * R + rel, return_counts=True)
        pairs, n_max = int(pair.numel()), int(cnt.max())
        Q_max, T_max = int(torch.bincount(pair // R).max()), int(torch.bincount(pair % R).max())
        del pair, cnt
        for F in [int(f) for f in args.widths.split(',')]:
            for B in [int(b) for b in args.blocks.split(',')]:
                for dtype in [getattr(torch, t) for t in args.dtypes.split(',')]:
                    ci = F // B
                    x = torch.randn((n, F), generator=g, device=dev).to(dtype).requires_grad_()
                    q = (torch.randn((R, B, ci, ci), generator=g, device=dev) / ci ** 0.5).to(dtype).requires_grad_()
                    gout = torch.randn((n, F), generator=g, device=dev).to(dtype)

                    def both(fn, x_, q_, g_):
                        out = fn(x_, q_)
                        return [out.detach()] + list(torch.autograd.grad(out, [x_, q_], g_))

                    # agreement on the timed inputs; S from the block call on absolute values (every term >= 0)
                    k, narrow = 2.0 ** -24 / U[dtype], int(dtype == torch.bfloat16)
                    cs = [(n_max + 2 * ci + Q_max + 2) * k + 2 * narrow, (d + 2 * ci + 3) * k + narrow,
                          (n_max + 2 * T_max + 3) * k + 2 * narrow]
                    ours_r = both(lambda a, b: adj.matmul_rel(a, b, rel), x, q, gout)
                    dense_r = both(lambda a, b: adj.matmul_rel(a, dense(b), rel), x, q, gout)
                    S = both(lambda a, b: adj.matmul_rel(a, b, rel), x.detach().abs().float().requires_grad_(),
                             q.detach().abs().float().requires_grad_(), gout.abs().float())
                    worst = [float(((a.double() - b.double()).abs() / (2 * c * U[dtype] * s.double()).clamp_min(1e-300)).max())
                             for a, b, s, c in zip(ours_r, dense_r, S, cs)]
                    assert max(worst) <= 1.0, 'blocks and dense differ by %s of the bound (out, grad_x, grad_Q)' % worst
                    del ours_r, dense_r, S

                    rec = {'bench': 'matmul_rel_blocks', 'graph': name, 'n': n, 'entries': E, 'R': R, 'pairs': pairs, 'F': F,
                           'B': B, 'dtype': str(dtype).replace('torch.', ''), 'device': torch.cuda.get_device_name(0),
                           'agreement': [round(w, 4) for w in worst]}
                    legs = {'fw': (lambda: adj.matmul_rel(x, q, rel).detach(), lambda: adj.matmul_rel(x, dense(q), rel).detach()),
                            'fwbw': (lambda: torch.autograd.grad(adj.matmul_rel(x, q, rel), [x, q], gout),
                                     lambda: torch.autograd.grad(adj.matmul_rel(x, dense(q), rel), [x, q], gout))}
                    for leg, (a, b) in legs.items():
                        rec[leg + '_ms'], rec[leg + '_ms_dense'] = timed_pair(a, b, args.repeat, args.warmup)
                        rec[leg + '_launches_dense'], rec[leg + '_launches'] = launches(b), launches(a)
                        rec[leg + '_peak_mib_dense'], rec[leg + '_peak_mib'] = peak_mib(b), peak_mib(a)
                    print(json.dumps(rec), flush=True)
                    with open(args.out, 'a') as fh:
                        fh.write(json.dumps(rec) + '\n')
                    del x, q, gout, legs
                    torch.cuda.empty_cache()
        del rel


if __name__ == '__main__':
    main()
