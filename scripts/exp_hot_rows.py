"""Would a side table of the sampled-hot rows of X replace the full relabelled copy?  Emulated with tensors, stock library.

For each sample stride the column ids hit by col[::stride] are "hot"; they get a slot behind X (x2 = cat([x, x[hot]]))
and every hot entry of col is redirected there (col2).  The hot ids' low bits are then uniform, so the shipped probe should
not fire on col2 and the merge kernel gathers in place: pre_ms shows whether it did.  Slot order: ascending id, or random.
Gate: merge(col2) - merge(parent) <= pre_ms(parent) / 4 for some stride with at most N / 4 hot rows."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pytorch_sparse_amd import _native as nat, synth
dev = torch.device('cuda:0')
scale, K = 21, 128
rowptr, col = synth.rmat_csr(scale, 20, seed=0, device=dev); n = 1 << scale
E = col.numel()
val = synth.values(E, device=dev); x = synth.features(n, K, device=dev)
def timeit(c, xx, tag):
    for _ in range(3): nat.spmm(rowptr, c, val, xx, 'sum')
    rows = []
    for _ in range(9):
        p = []
        s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
        s.record(); nat.spmm(rowptr, c, val, xx, 'sum'); e.record(); e.synchronize()
        nat.spmm(rowptr, c, val, xx, 'sum', profile=p)
        rows.append((s.elapsed_time(e), p[0], p[1], p[2]))
    med = [sorted(r[i] for r in rows)[len(rows) // 2] for i in range(4)]
    print('%-44s call %.3f  pre %.3f  merge %.3f  fixup %.3f ms' % ((tag, ) + tuple(med)), flush=True)
    return med
ref, _ = nat.spmm(rowptr, col, val, x, 'sum')
base = timeit(col, x, 'parent (probe fires, full copy)')
g = torch.Generator(device=dev); g.manual_seed(1)
for stride in (128, 32, 8):
    hot = torch.zeros(n, dtype=torch.bool, device=dev)
    hot[col[::stride]] = True
    ids = hot.nonzero().flatten(); H = ids.numel()
    left = 1.0 - float(hot[col].float().mean())
    for order in ('ascending', 'random'):
        slot = torch.zeros(n, dtype=torch.int64, device=dev)
        place = torch.arange(H, device=dev) if order == 'ascending' else torch.randperm(H, generator=g, device=dev)
        slot[ids] = place
        x2 = torch.empty(n + H, K, device=dev); x2[:n] = x; x2[n + place] = x[ids]
        col2 = torch.where(hot[col], n + slot[col], col)
        out, _ = nat.spmm(rowptr, col2, val, x2, 'sum')
        assert torch.equal(out, ref) or torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
        m = timeit(col2, x2, '1/%d: %d hot (%.1f %% of N, %d MB), %.1f %% left, %s' %
                   (stride, H, 100.0 * H / n, H * K * 4 >> 20, 100 * left, order))
        print('    merge - parent merge = %+.3f ms; gate %.3f ms (parent pre / 4); N/4 rows: %s' %
              (m[2] - base[2], base[1] / 4, 'yes' if 4 * H <= n else 'NO'), flush=True)
        del x2, col2, slot
timeit(col, x, 'parent (repeat)')
