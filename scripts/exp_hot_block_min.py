"""Stage times of one build on the north star (medians of 9 via profile=): call, prologue, merge kernel, fix-up.
The library is the one TSAMD_LIB names (a build with -DTSAMD_HOT_BLOCK_MIN=8 / 16 / 32, or the parent's), so one
process per build; argv[1] is the label printed in front."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pytorch_sparse_amd import _native as nat, synth
dev = torch.device('cuda:0')
scale, K = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (21, 128)
ef = int(sys.argv[4]) if len(sys.argv) > 4 else 20
rowptr, col = synth.rmat_csr(scale, ef, seed=0, device=dev); n = 1 << scale
val = synth.values(col.numel(), device=dev); x = synth.features(n, K, device=dev)
for _ in range(3): nat.spmm(rowptr, col, val, x, 'sum')
rows = []
for _ in range(9):
    p = []
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record(); nat.spmm(rowptr, col, val, x, 'sum'); e.record(); e.synchronize()
    nat.spmm(rowptr, col, val, x, 'sum', profile=p)
    rows.append((s.elapsed_time(e), p[0], p[1], p[2]))
med = [sorted(r[i] for r in rows)[len(rows) // 2] for i in range(4)]
print('%-10s scale %d ef %d F %d: call %.3f  pre %.3f  merge %.3f  fixup %.3f ms' % ((sys.argv[1], scale, ef, K) + tuple(med)), flush=True)
