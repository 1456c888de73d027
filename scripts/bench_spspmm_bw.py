"""SpSpMM value gradients: forward, gA alone, gB alone, both, and torch.sparse.mm forward + backward on the same device
and in the same process, as HIP-event medians after warm-up.  One JSON line per shape, appended to
profiles/spspmm_bw_bench.jsonl.

  c4      config 4 of tests/baseline_configs.py: A * A^T, 500 k x 500 k, ~15 entries per row (~120 M products)
  rmat16  symmetrised R-MAT scale 16, edge factor 8: A * A (hub rows, products explode quadratically)

usage: python scripts/bench_spspmm_bw.py [c4] [rmat16] [--iters N]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pytorch_sparse_amd as ts  # noqa: E402
from pytorch_sparse_amd import synth  # noqa: E402
from tests import baseline_configs as bc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'spspmm_bw_bench.jsonl')


def operands(kind, dev):
    if kind == 'c4':
        return bc.spspmm_inputs(dev, 'c4')
    row, col = synth.rmat_edges(16, 8, seed=0, device=dev)
    n = 1 << 16
    r, c = torch.cat([row, col]), torch.cat([col, row])
    A = ts.SparseTensor(row=r, col=c, sparse_sizes=(n, n)).coalesce()
    A = A.set_value(synth.values(A.nnz(), device=dev), layout='coo')
    return A, A


def run(kind, dev, iters):
    A, B = operands(kind, dev)
    rpA, cA, vA = A.csr()
    rpB, cB, vB = B.csr()
    A.storage.colptr()
    A.storage.csr2csc()  # the column view of A is cached, as it is on a tensor that has been transposed or multiplied
    N = B.sparse_size(1)
    res = dict(shape=kind, m=A.sparse_size(0), k=A.sparse_size(1), n=N, nnzA=cA.numel(), nnzB=cB.numel(), iters=iters,
               device=torch.cuda.get_device_name(dev))

    def fwd(a, b):
        return torch.ops.tsamd.spspmm(rpA, cA, a, rpB, cB, b, N, True, A.storage._colptr, A.storage._csr2csc)

    with torch.no_grad():
        res['forward_ms'] = bc.gpu_ms(lambda: fwd(vA, vB), iters=iters)
    a, b = vA.clone().requires_grad_(True), vB.clone().requires_grad_(True)
    rpC, cC, vC = fwd(a, b)
    res['nnzC'] = cC.numel()
    lens = (rpB[1:] - rpB[:-1])[cA]
    res['products'] = int(lens.sum())
    g = synth.values(vC.numel(), seed=5, device=dev)
    res['gA_ms'] = bc.gpu_ms(lambda: torch.autograd.grad(vC, [a], g, retain_graph=True), iters=iters)
    res['gB_ms'] = bc.gpu_ms(lambda: torch.autograd.grad(vC, [b], g, retain_graph=True), iters=iters)
    res['both_ms'] = bc.gpu_ms(lambda: torch.autograd.grad(vC, [a, b], g, retain_graph=True), iters=iters)
    res['backward_over_forward'] = res['both_ms'] / res['forward_ms']
    del vC, rpC, cC, g

    # the reference's route: torch.sparse.mm, differentiable in both value tensors
    try:
        ia = torch.stack([A.storage.row(), cA])
        ib = torch.stack([B.storage.row(), cB])
        ta, tb = vA.clone().requires_grad_(True), vB.clone().requires_grad_(True)

        def ref_fwd():
            SA = torch.sparse_coo_tensor(ia, ta, (res['m'], res['k']), is_coalesced=True)
            SB = torch.sparse_coo_tensor(ib, tb, (res['k'], res['n']), is_coalesced=True)
            return torch.sparse.mm(SA, SB)

        def ref_fwbw():
            C = ref_fwd()
            v = C.coalesce().values()
            torch.autograd.grad(v, [ta, tb], torch.ones_like(v))

        with torch.no_grad():
            res['torch_sparse_mm_forward_ms'] = bc.gpu_ms(ref_fwd, iters=min(iters, 3), warm=1)
        res['torch_sparse_mm_fwbw_ms'] = bc.gpu_ms(ref_fwbw, iters=min(iters, 3), warm=1)
    except Exception as e:  # unsupported on the device, or out of memory: record what it said
        res['torch_sparse_mm_error'] = '%s: %s' % (type(e).__name__, str(e).splitlines()[0][:300])
    return res


def main():
    args = [x for x in sys.argv[1:] if x in ('c4', 'rmat16')]
    iters = int(sys.argv[sys.argv.index('--iters') + 1]) if '--iters' in sys.argv else 7
    dev = torch.device('cuda:0')
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for kind in args or ['c4', 'rmat16']:
        res = run(kind, dev, iters)
        line = json.dumps(res)
        print(line, flush=True)
        with open(OUT, 'a') as f:
            f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
