"""What holding the features as fp8 codes buys the gather: ``adj.matmul_q8(xq, scale)`` (csrc/spmm_q8.hip) against
``adj.matmul(x)`` with x in bfloat16 and in float32 -- the same graph, process and device, one call of each in turn,
HIP-event medians of --repeat calls after --warmup -- and ``quantize_rows`` alone.  reduce is sum, with and without
values.

Before a case is timed the fp8 product must agree with either matmul: per element within the bound of
tests/test_spmm_q8_gpu.py for both sides, plus the quantisation of the inputs, 2^-4 relative for e4m3 (half an ulp of 3
mantissa bits; against the bfloat16 call 2^-7 more for its inputs and 2^-8 |out| for its store), all over
sum_e |value[e] x[col[e], f]|.  'gate_f32' / 'gate_bf16' are the worst error over that bound; a case above 1 is
reported with 'parity': false and not timed.  2^-4 relative holds for NORMAL codes only: an element below 2^-6 scale
is coded as a subnormal, with an error of up to 2^-10 scale whatever its size, and a row of one such entry misses the
gate (measured: 4.7 times the bound on rmat_scale14_ef20 at F = 32, 0.94 with the term 2^-10 sum_e |value| scale
added).  The features are therefore standard normal with |x| < 1e-3 moved to +-1e-3, which no row of up to 1024
normal draws codes as a subnormal; --randn leaves them as drawn.  Timings do not depend on the values.

Appends one JSON line per (graph, F, values) to --out; --table prints the README table of a results file.

    python scripts/bench_spmm_q8.py [--repeat 20] [--warmup 3] [--small]
    python scripts/bench_spmm_q8.py --table profiles/spmm_q8_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

from bench_attention import timed  # noqa: E402


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['graph', 'F', 'values', 'matmul float32', 'matmul bfloat16', 'matmul_q8 (fp8)', 'bfloat16 / fp8',
            'quantize_rows']
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        if not r['parity']:
            cells = ['parity gate missed: not timed'] + [''] * 4
        else:
            cells = ['%.3g ms' % r['f32_ms'], '%.3g ms' % r['bf16_ms'],
                     '%.3g ms%s' % (r['q8_ms'], ' (slower)' if r['q8_ms'] > r['bf16_ms'] else ''),
                     '%.2f' % (r['bf16_ms'] / r['q8_ms']), '%.3g ms' % r['quantize_ms']]
        print('| ' + ' | '.join([r['graph'], str(r['F']), 'yes' if r['values'] else 'no'] + cells) + ' |')


def in_turn(fns, repeat, warmup):
    """medians (ms) of `repeat` calls of every function, one call of each in turn"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(repeat):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--graphs', default='0,1,2', help='which of the three graphs to run')
    ap.add_argument('--widths', default='32,64,128,256')
    ap.add_argument('--randn', action='store_true', help='plain standard-normal features (see the gate above)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spmm_q8_bench.jsonl'))
    ap.add_argument('--table', metavar='JSONL', help='print the README table of a results file and exit')
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    import pytorch_sparse_amd as ts
    from pytorch_sparse_amd import synth
    assert torch.cuda.is_available(), 'the benchmark needs a GPU'
    dev = torch.device('cuda:0')
    big, mid = (14, 13) if args.small else (21, 20)
    graphs = [('rmat_scale%d_ef20' % big, lambda: synth.rmat_csr(big, 20, seed=0, device=dev)),
              ('rmat_scale%d_ef20' % mid, lambda: synth.rmat_csr(mid, 20, seed=0, device=dev)),
              ('uniform_deg20_2^%d' % big, lambda: synth.uniform_degree_csr(1 << big, 1 << big, 20, device=dev))]
    for name, make in [graphs[int(i)] for i in args.graphs.split(',')]:
        rowptr, col = make()
        n, E = rowptr.numel() - 1, int(col.numel())
        deg = (rowptr[1:] - rowptr[:-1]).float()[:, None]
        g = torch.Generator(device=dev).manual_seed(1)
        weights = torch.rand(E, generator=g, device=dev) + 0.5
        for F in (int(f) for f in args.widths.split(',')):
            x = torch.randn((n, F), generator=g, device=dev)
            if not args.randn:  # below 2^-6 scale (< 2.2e-4 here) a code is subnormal and 2^-4 relative does not hold
                x = torch.where(x.abs() < 1e-3, torch.copysign(torch.full_like(x, 1e-3), x), x)
            xb = x.bfloat16()
            xq, scale = ts.quantize_rows(x)
            for with_value in (False, True):
                def adj(v):
                    return ts.SparseTensor(rowptr=rowptr, col=col, value=v, sparse_sizes=(n, n), is_sorted=True,
                                           trust_data=True)
                a32 = adj(weights if with_value else None)
                ab = adj(weights.bfloat16() if with_value else None)
                fns = {'q8': lambda: a32.matmul_q8(xq, scale), 'bf16': lambda: ab.matmul(xb), 'f32': lambda: a32.matmul(x)}
                # the parity gate: the fp8 product against either matmul, worst error over its bound
                out_q, absum = fns['q8'](), a32.matmul(x.abs())
                rounding = 2 * (deg + 3) * 2.0 ** -24
                tiny = torch.finfo(torch.float32).tiny
                err = (out_q - fns['f32']()).abs()
                gate_f32 = (err / ((2.0 ** -4 + rounding) * absum).clamp(min=tiny)).max()
                out_b = fns['bf16']().float()
                tol_b = (2.0 ** -4 + 2.0 ** -7 + rounding) * absum + 2.0 ** -8 * out_b.abs()
                gate_bf16 = ((out_q - out_b).abs() / tol_b.clamp(min=tiny)).max()
                rec = {'bench': 'spmm_q8', 'graph': name, 'n': n, 'entries': E, 'F': F, 'values': with_value,
                       'gate_f32': round(float(gate_f32), 4), 'gate_bf16': round(float(gate_bf16), 4),
                       'device': torch.cuda.get_device_name(0)}
                rec['parity'] = rec['gate_f32'] <= 1 and rec['gate_bf16'] <= 1
                del out_q, absum, out_b, tol_b
                if rec['parity']:
                    for k, ms in in_turn(fns, args.repeat, args.warmup).items():
                        rec[k + '_ms'] = ms
                    rec['quantize_ms'] = timed(lambda: ts.quantize_rows(x), args.repeat, args.warmup)
                    rec['bf16_over_q8'] = round(rec['bf16_ms'] / rec['q8_ms'], 3)
                print(json.dumps(rec), flush=True)
                with open(args.out, 'a') as fh:
                    fh.write(json.dumps(rec) + '\n')
                torch.cuda.empty_cache()
            del x, xb, xq, scale
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
