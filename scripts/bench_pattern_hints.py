"""Two timings behind docs/design/spmm_forward.md, "Pattern hints", each printing one JSON line.  Run it from the root
of the tree to measure (the package is imported from the working directory), so that the same file times two builds:

    python scripts/bench_pattern_hints.py control   uniform control graph (bench.py's control_graph shape): the C-ABI call,
                                                    which keeps no hints, and the torch op, single calls and queued
    python scripts/bench_pattern_hints.py first     first sighting: six R-MAT patterns of the headline shape in rotation
                                                    through the op -- with four cache entries every call builds its hints
"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import pytorch_sparse_amd  # noqa: E402,F401
from pytorch_sparse_amd import _native as nat, synth  # noqa: E402
from tests import baseline_configs as bc  # noqa: E402

dev = torch.device('cuda:0')
hints = torch.ops.tsamd.pattern_hints if hasattr(torch.ops.tsamd, 'pattern_hints') else None  # (absent in older builds)


def control():
    m, deg, F = 1 << 21, 20, 128
    rp, c = synth.uniform_degree_csr(m, m, deg, seed=5, device=dev)
    v = synth.values(c.numel(), seed=6, device=dev)
    x = synth.features(m, F, seed=7, device=dev)
    op = lambda: torch.ops.torch_sparse.spmm_sum(None, rp, c, v, None, None, x)  # noqa: E731
    return dict(edges=c.numel(), cabi_ms=round(bc.gpu_ms(lambda: nat.spmm(rp, c, v, x, 'sum'), iters=10), 4),
                op_ms=round(bc.gpu_ms(op, iters=10), 4), op_stream_ms=round(bc.gpu_ms_stream(op, iters=50, warm=5), 4))


def first():
    scale, ef, F = 21, 20, 128
    pats = [synth.rmat_csr(scale, ef, seed=100 + i, device=dev) for i in range(6)]
    vals = [synth.values(c.numel(), seed=1, device=dev) for _, c in pats]
    x = synth.features(1 << scale, F, seed=2, device=dev)

    def call(i):
        return torch.ops.torch_sparse.spmm_sum(None, pats[i][0], pats[i][1], vals[i], None, None, x)
    for i in range(6):
        call(i)
    torch.cuda.synchronize()
    before = hints() if hints else None
    ts = []
    for _ in range(5):
        for i in range(6):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            call(i)
            e.record()
            e.synchronize()
            ts.append(s.elapsed_time(e))
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        for i in range(6):
            call(i)
    e.record()
    e.synchronize()
    r = dict(calls=len(ts), median_ms=round(sorted(ts)[len(ts) // 2], 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
             stream_mean_ms=round(s.elapsed_time(e) / 30, 4))
    if hints:
        after = hints()
        r['builds'], r['reuses'] = after[1] - before[1], after[2] - before[2]
    return r


if __name__ == '__main__':
    with torch.no_grad():
        print(json.dumps(control() if sys.argv[1:] == ['control'] else first()))
