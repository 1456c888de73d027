"""ego_k_hop_sample_adj (ShaDow-GNN's sampler) on one MI355X: R-MAT scale 20, edge factor 20 (the config-2 graph).
Wall time of the op including its host read-backs, median of 7 after 2 warm-up calls.  The reference has this op on
the CPU only and oracle/_ref does not build it: GPU numbers only.  Prints one JSON object per line:
  nodes   sum |S_g| (length of n_id)
  V       candidate entries of the induced step (every stored entry of every row of n_id)
  edges   output entries (length of col)
  syncs   host read-backs of one call (torch's sync debug mode warns on each)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pytorch_sparse_amd  # noqa: E402,F401
from pytorch_sparse_amd import synth  # noqa: E402

dev = torch.device('cuda:0')


def wall(fn, iters=7, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2] * 1e3


def count_syncs(fn):
    import tempfile
    torch.cuda.synchronize()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as tmp:
        os.dup2(tmp.fileno(), 2)
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        # (not the bare word: torch's one-time notice that the debug mode is a prototype contains it too)
        return tmp.read().decode(errors='replace').count('called a synchronizing')


scale = int(os.environ.get('SCALE', 20))
rp, c = synth.rmat_csr(scale, 20, seed=0, device=dev)
n = 1 << scale
deg = rp[1:] - rp[:-1]
perm = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(dev)

for seeds, depth, k, replace in ((1024, 2, 5, False), (1024, 2, 10, False), (8192, 2, 10, False), (1024, 3, 5, False),
                                 (8192, 2, 10, True)):
    idx = perm[:seeds]
    fn = lambda: torch.ops.torch_sparse.ego_k_hop_sample_adj(rp, c, idx, depth, k, replace)  # noqa: E731
    ms = wall(fn)
    torch.manual_seed(0)
    out_rp, out_c, n_id, e_id, ptr, root = fn()
    V = int(deg[n_id].sum())
    print(json.dumps(dict(bench='ego_k_hop_sample_adj', scale=scale, seeds=seeds, depth=depth, k=k, replace=replace,
                          ms=round(ms, 3), nodes=n_id.numel(), V=V, edges=out_c.numel(), syncs=count_syncs(fn))),
          flush=True)
