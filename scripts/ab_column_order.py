"""Merge-kernel time of one SpMM call under tsamd_spmm_column_order 0 / 1 / 2 (off, auto, forced), interleaved in one
process: python scripts/ab_column_order.py [reps] [scale] [edge_factor] [F].  Prints prologue / merge / fix-up medians
(tsamd_spmm_profiled, HIP events) and checks that the three outputs are equal in every bit.  TSAMD_LIB selects another
build of libtsamd.so (e.g. one compiled with an experimental layout) for the same comparison."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sparse_amd import _native as nat, synth  # noqa: E402

reps, scale, ef, F = (int(a) for a in (sys.argv[1:5] + ['12', '21', '20', '128'][len(sys.argv) - 1:]))
dev = torch.device('cuda:0')
L = nat.lib()
rp, c = synth.rmat_csr(scale, ef, seed=0, device=dev)
v = synth.values(c.numel(), seed=1, device=dev)
x = synth.features(1 << scale, F, seed=2, device=dev)
res, outs = {0: [], 1: [], 2: []}, {}
for rep in range(reps + 2):
    for s in (0, 1, 2):
        L.tsamd_spmm_column_order(s)
        prof = []
        out, _ = nat.spmm(rp, c, v, x, 'sum', profile=prof)
        res[s].append(prof)
        if rep == 0:
            outs[s] = out.clone()
L.tsamd_spmm_column_order(1)
for s in (1, 2):
    print('setting %d equals setting 0 in every bit: %s' % (s, torch.equal(outs[0].view(torch.int32), outs[s].view(torch.int32))))
for s in (0, 1, 2):
    a = np.array(res[s][2:])
    print('setting %d  prologue / merge / fix-up median ms %s  merge min .. max %.4f .. %.4f'
          % (s, np.median(a, 0).round(4).tolist(), a[:, 1].min(), a[:, 1].max()))
