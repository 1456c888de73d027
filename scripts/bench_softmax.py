"""Timings of SparseTensor.softmax(1) (csrc/softmax.hip) against the composition it replaces, written out below from
the parts the package had before: adj.max(dim=1), ptr2ind, a gather, exp, adj.sum(dim=1), another gather and a divide
(the maximum is part of the autograd graph, as a user of those parts would have written it).  One process, one device;
HIP-event medians of --repeat calls after --warmup; forward alone, and forward + backward of the values.  Graphs: the
north-star R-MAT (scale 21, edge factor 20), the R-MAT of BASELINE.json configs[2] (scale 20, edge factor 20) and a
uniform degree-20 control of the north star's size, each with D = 1 and D = 8 heads in fp32 and bf16.  Appends one JSON
line per (graph, D, dtype) to --out: milliseconds of both routes, launches per call, and the achieved bytes/s of the
forward against its algorithmic bytes 2 * itemsize * E * D + 8 * (nseg + 1).

    python scripts/bench_softmax.py [--repeat 20] [--warmup 3] [--small] [--out profiles/softmax_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pytorch_sparse_amd as ts  # noqa: E402
from pytorch_sparse_amd import synth  # noqa: E402
from pytorch_sparse_amd.segment import segment_reduce  # noqa: E402


def composed_softmax(value, rowptr, nseg):
    """The only route before tsamd::segment_softmax: seven launches, about seven passes over the values."""
    m = segment_reduce(value, None, rowptr, nseg, 'max', balanced=True)
    row = torch.ops.torch_sparse.ptr2ind(rowptr, value.size(0))
    e = (value - m.index_select(0, row)).exp()
    s = segment_reduce(e, None, rowptr, nseg, 'sum', balanced=True)
    return e / s.index_select(0, row)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--small', action='store_true', help='scale-14 graphs (a quick look)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'softmax_bench.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    big, mid = (14, 13) if args.small else (21, 20)
    graphs = [('rmat_scale%d_ef20' % big, lambda: synth.rmat_csr(big, 20, seed=0, device=dev)),
              ('rmat_scale%d_ef20' % mid, lambda: synth.rmat_csr(mid, 20, seed=0, device=dev)),
              ('uniform_deg20_2^%d' % big, lambda: synth.uniform_degree_csr(1 << big, 1 << big, 20, device=dev))]
    for name, make in graphs:
        rowptr, col = make()
        n, E = rowptr.numel() - 1, int(col.numel())
        adj0 = ts.SparseTensor(rowptr=rowptr, col=col, sparse_sizes=(n, n), is_sorted=True, trust_data=True)
        longest = int((rowptr[1:] - rowptr[:-1]).max())
        for D in (1, 8):
            for dtype in (torch.float32, torch.bfloat16):
                g = torch.Generator(device=dev).manual_seed(1)
                shape = (E, ) if D == 1 else (E, D)
                value = (torch.randn(shape, generator=g, device=dev) * 4).to(dtype)
                gout = torch.randn(shape, generator=g, device=dev).to(dtype)
                adj = adj0.set_value(value, layout='coo')
                ours = lambda: adj.softmax(1).storage.value()  # noqa: E731
                theirs = lambda: composed_softmax(value, rowptr, n)  # noqa: E731
                err = float((ours().double() - theirs().double()).abs().max())
                vg = value.clone().requires_grad_()
                adj_g = adj0.set_value(vg, layout='coo')
                ours_fb = lambda: torch.autograd.grad(adj_g.softmax(1).storage.value(), vg, gout)  # noqa: E731
                theirs_fb = lambda: torch.autograd.grad(composed_softmax(vg, rowptr, n), vg, gout)  # noqa: E731
                nbytes = 2 * value.element_size() * E * D + 8 * (n + 1)
                rec = {'bench': 'softmax', 'graph': name, 'n': n, 'entries': E, 'longest_row': longest, 'D': D,
                       'dtype': str(dtype).replace('torch.', ''), 'device': torch.cuda.get_device_name(0),
                       'fw_ms': timed(ours, args.repeat, args.warmup),
                       'fw_ms_composed': timed(theirs, args.repeat, args.warmup),
                       'fwbw_ms': timed(ours_fb, args.repeat, args.warmup),
                       'fwbw_ms_composed': timed(theirs_fb, args.repeat, args.warmup),
                       'fw_launches': launches(ours), 'fw_launches_composed': launches(theirs),
                       'fwbw_launches': launches(ours_fb), 'fwbw_launches_composed': launches(theirs_fb),
                       'fw_bytes': nbytes, 'max_abs_diff_of_routes': err}
                rec['fw_gbps'] = round(nbytes / rec['fw_ms'] / 1e6, 1)
                rec['fw_gbps_composed'] = round(nbytes / rec['fw_ms_composed'] / 1e6, 1)
                rec['fw_speedup'] = round(rec['fw_ms_composed'] / rec['fw_ms'], 2)
                rec['fwbw_speedup'] = round(rec['fwbw_ms_composed'] / rec['fwbw_ms'], 2)
                print(json.dumps(rec), flush=True)
                with open(args.out, 'a') as fh:
                    fh.write(json.dumps(rec) + '\n')
                del value, gout, adj, vg, adj_g
        del adj0, rowptr, col
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
