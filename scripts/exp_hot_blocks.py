"""Would whole 64-id blocks serve as the unit of the hot table instead of single ids?  Emulated with tensors, stock library.

The flags are the shipped ones (flag[col[::32]] = 1).  A block of 64 consecutive ids is selected when at least T of its ids
are flagged; the selected blocks get 64 consecutive slots each behind X (x2 = cat([x, appendix])), in block order, and every
entry of col that names an id of a selected block is redirected there (col2).  Slot of id in the block of rank r:
r * 64 + ((id + rot(r)) & 63).  "rotated": rot(r) = top six bits of r * 0x9E3779B1 (an odd multiplier), so that the popular
low-bit patterns of consecutive blocks land on different offsets.  "aligned": rot = 21 for every block -- adding a constant is
a bijection on every low-bit class, so the popular ids of all blocks still share their classes exactly as with rot = 0, but
the shipped probe (which tests (c & 7) == 0 and (c & 63) == 0) does not fire on col2 and lay a per-id table over the
emulation.  pre_ms shows whether it stayed quiet (probe + partition only: ~0.03 ms).
Gate: merge(col2) - merge(shipped per-id route, same process) <= +0.03 ms for T = 16 or its better neighbour."""
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
    print('%-58s call %.3f  pre %.3f  merge %.3f  fixup %.3f ms' % ((tag, ) + tuple(med)), flush=True)
    return med
ref, _ = nat.spmm(rowptr, col, val, x, 'sum')
base = timeit(col, x, 'shipped (probe fires, per-id hot table)')
flag = torch.zeros(n, dtype=torch.bool, device=dev)
flag[col[::32]] = True
print('flagged ids: %d (%.1f %% of N), %.1f %% of the gathers left in place by the per-id table' %
      (int(flag.sum()), 100.0 * float(flag.float().mean()), 100.0 * (1.0 - float(flag[col].float().mean()))), flush=True)
per_block = flag.view(-1, 64).sum(1)
blk = col >> 6
for T in (8, 16, 32):
    sel = per_block >= T
    S = int(sel.sum())
    rank = torch.cumsum(sel.long(), 0) - sel.long()  # exclusive scan: the block's rank among the selected ones
    left = 1.0 - float(sel[blk].float().mean())
    ids = (sel.nonzero().flatten()[:, None] * 64 + torch.arange(64, device=dev)[None, :]).flatten()  # rows of the selected blocks
    for mode in ('aligned', 'rotated'):
        rot = ((rank * 0x9E3779B1) & 0xFFFFFFFF) >> 26 if mode == 'rotated' else torch.full_like(rank, 21)
        slot = lambda i: rank[i >> 6] * 64 + ((i + rot[i >> 6]) & 63)
        x2 = torch.empty(n + 64 * S, K, device=dev); x2[:n] = x; x2[n + slot(ids)] = x[ids]
        col2 = torch.where(sel[blk], n + slot(col), col)
        out, _ = nat.spmm(rowptr, col2, val, x2, 'sum')
        assert torch.equal(out, ref) or torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
        m = timeit(col2, x2, 'T = %d: %d blocks (%.1f %% of N, %d MB), %.1f %% left, %s' %
                   (T, S, 100.0 * S * 64 / n, S * 64 * K * 4 >> 20, 100 * left, mode))
        print('    merge - shipped merge = %+.3f ms; gate +0.030 ms; probe quiet: %s' %
              (m[2] - base[2], 'yes' if m[1] < base[1] / 2 else 'NO'), flush=True)
        del x2, col2
timeit(col, x, 'shipped (repeat)')
