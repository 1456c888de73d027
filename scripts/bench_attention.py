"""Timings of SparseTensor.sddmm / matmul_heads (csrc/sddmm.hip, csrc/spmm_heads.hip) against the compositions they
replace, written out below from the parts the package had before:

    scores       (q[row] * k[col]).sum(-1) * scale                       two [nnz, H, D] gathers
    aggregation  a loop over the heads of adj.set_value(v[:, h].contiguous(), layout='coo').matmul(x[:, h]), stacked
    layer        scores -> adj.softmax(1) -> aggregation, forward and forward + backward w.r.t. q, k and v

One process, one device; HIP-event medians of --repeat calls after --warmup.  Graphs: the three of
scripts/bench_softmax.py (north-star R-MAT scale 21, the R-MAT of BASELINE.json configs[2], a uniform degree-20 control),
each at (H, D) = (1, 64), (8, 16), (8, 64) in fp32 and bf16.  A composition whose [nnz, H, D] temporaries (three in the
forward, five with the backward) would not fit --memory-gb of device memory is not run (null in the record).  Appends
one JSON line per (graph, H, D, dtype) to --out; --table prints the README table of a results file.

    python scripts/bench_attention.py [--repeat 20] [--warmup 3] [--small] [--out profiles/attention_bench.jsonl]
    python scripts/bench_attention.py --table profiles/attention_bench.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = (('sddmm', 'scores'), ('matmul_heads', 'aggregation'), ('layer_fw', 'layer forward'),
         ('layer_fwbw', 'layer forward + backward'))


def timed(fn, repeat, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return round(ms[len(ms) // 2], 4)


def launches(fn):
    """Kernels one call launches (torch.profiler); None where the profiler cannot say."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(ev.device_type).endswith('CUDA') and 'emcpy' not in ev.name)
        return n or None
    except Exception:  # noqa: BLE001
        return None


def table(path):
    recs = [json.loads(line) for line in open(path) if line.strip()]
    head = ['graph', 'H x D', 'dtype']
    for key, title in PAIRS:
        head += [title + ': composition', title + ': now']
    head.append('launches (scores, aggregation, layer fw, fw + bw): composition -> now')
    print('| ' + ' | '.join(head) + ' |')
    print('|' + '---|' * len(head))
    for r in recs:
        cells = [r['graph'], '%d x %d' % (r['H'], r['D']), r['dtype']]
        for key, _ in PAIRS:
            ours, theirs = r[key + '_ms'], r[key + '_ms_composed']
            cells.append('does not fit' if theirs is None else '%.3g ms' % theirs)
            cells.append('%.3g ms%s' % (ours, ' (slower)' if theirs is not None and ours > theirs else ''))
        cells.append(', '.join('%s -> %s' % (r[key + '_launches_composed'], r[key + '_launches']) for key, _ in PAIRS))
        print('| ' + ' | '.join(cells) + ' |')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--memory-gb', type=float, default=200.0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'attention_bench.jsonl'))
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
    for name, make in graphs:
        rowptr, col = make()
        n, E = rowptr.numel() - 1, int(col.numel())
        adj = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
        row = adj.storage.row()
        adj.storage.colptr(), adj.storage.csr2csc()  # the caches of a training loop's second step
        longest = int((rowptr[1:] - rowptr[:-1]).max())
        for H, D in ((1, 64), (8, 16), (8, 64)):
            for dtype in (torch.float32, torch.bfloat16):
                g = torch.Generator(device=dev).manual_seed(1)
                q, k, v = (torch.randn((n, H, D), generator=g, device=dev).to(dtype) for _ in range(3))
                p = torch.rand((E, H), generator=g, device=dev).to(dtype)
                gout = torch.randn((n, H, D), generator=g, device=dev).to(dtype)
                scale = D ** -0.5
                fits = 3 * E * H * D * q.element_size() <= args.memory_gb * 2 ** 30
                fits_bw = 5 * E * H * D * q.element_size() <= args.memory_gb * 2 ** 30

                def scores_composed(q=q, k=k):
                    return (q[row] * k[col]).sum(-1) * scale

                def heads_composed(p, v=v):
                    return torch.stack([adj.set_value(p[:, h].contiguous(), layout='coo').matmul(v[:, h])
                                        for h in range(H)], 1)

                def layer(q=q, k=k, v=v):
                    return adj.sddmm(q, k, scale).softmax(1).matmul_heads(v)

                def layer_composed(q=q, k=k, v=v):
                    s = adj.set_value(scores_composed(q, k), layout='coo').softmax(1).storage.value()
                    return heads_composed(s, v)

                ap_ = adj.set_value(p, layout='coo')
                gq, gk, gv = (t.clone().requires_grad_() for t in (q, k, v))
                calls = {
                    'sddmm': (lambda: adj.sddmm(q, k, scale), scores_composed if fits else None),
                    'matmul_heads': (lambda: ap_.matmul_heads(v), lambda: heads_composed(p)),
                    'layer_fw': (layer, layer_composed if fits else None),
                    'layer_fwbw': (lambda: torch.autograd.grad(layer(gq, gk, gv), (gq, gk, gv), gout),
                                   (lambda: torch.autograd.grad(layer_composed(gq, gk, gv), (gq, gk, gv), gout))
                                   if fits_bw else None),
                }
                rec = {'bench': 'attention', 'graph': name, 'n': n, 'entries': E, 'longest_row': longest, 'H': H,
                       'D': D, 'dtype': str(dtype).replace('torch.', ''), 'device': torch.cuda.get_device_name(0)}
                for key, (ours, theirs) in calls.items():
                    rec[key + '_ms'] = timed(ours, args.repeat, args.warmup)
                    rec[key + '_launches'] = launches(ours)
                    rec[key + '_ms_composed'] = rec[key + '_launches_composed'] = rec[key + '_speedup'] = None
                    if theirs is not None:
                        rec[key + '_ms_composed'] = timed(theirs, args.repeat, args.warmup)
                        rec[key + '_launches_composed'] = launches(theirs)
                        rec[key + '_speedup'] = round(rec[key + '_ms_composed'] / rec[key + '_ms'], 2)
                    torch.cuda.empty_cache()
                if fits:
                    rec['max_abs_diff_of_layers'] = float((layer().double() - layer_composed().double()).abs().max())
                print(json.dumps(rec), flush=True)
                with open(args.out, 'a') as fh:
                    fh.write(json.dumps(rec) + '\n')
                del q, k, v, p, gout, gq, gk, gv, ap_, calls
                torch.cuda.empty_cache()
        del adj, row, rowptr, col
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
