"""Reverse Cuthill-McKee reordering (reference: torch_sparse/bandwidth.py).  The reference hands the matrix to
``scipy.sparse.csgraph.reverse_cuthill_mckee`` on the host; here the ordering is computed on the GPU
(csrc/rcm.hip, docs/design/rcm.md) and equals scipy's permutation element by element.  Tensors that are not on
the GPU take the reference's scipy path unchanged."""
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .select import permute
from .tensor import SparseTensor


def _scipy_seed_order(deg: Tensor, nnz: int) -> Tensor:
    """The order in which scipy tries the nodes as component seeds: ``numpy.argsort`` of the degrees with the
    DEFAULT kind, on the index dtype scipy gives a matrix of this size.  That sort is not stable, and the order
    it leaves equal degrees in belongs to the numpy build, so only the same call reproduces it."""
    dtype = np.int32 if max(deg.numel(), nnz) < 2 ** 31 else np.int64
    order = np.argsort(deg.cpu().numpy().astype(dtype))
    return torch.from_numpy(order.astype(np.int64)).to(deg.device)


def reverse_cuthill_mckee(src: SparseTensor, is_symmetric: Optional[bool] = None, *,
                          seeds: str = 'scipy') -> Tuple[SparseTensor, Tensor]:
    """-> (src permuted, perm).  On the GPU the breadth-first search, the symmetrisation before it and the
    permutation after it are HIP kernels, and the matrix never leaves the device.

    seeds='scipy' (default): ONE host step remains -- the degree vector (N integers, not the matrix) is copied to
    the host, ``numpy.argsort``-ed and the order copied back.  It is there for bit-compatibility: scipy picks the
    start node of every component in the order of an unstable sort of the degrees, so which of several nodes of
    equal degree comes first is decided by numpy's sort and nothing else reproduces it.  With it, ``perm`` equals
    ``scipy.sparse.csgraph.reverse_cuthill_mckee(..., symmetric_mode=True)`` element by element.
    seeds='stable': the seeds are tried in (degree, id) order, built on the device: no host step, and a result
    that does not depend on the numpy build.  An equally good ordering, different from scipy's where degrees tie."""
    if seeds not in ('scipy', 'stable'):
        raise ValueError("seeds must be 'scipy' or 'stable'")
    if is_symmetric is None:
        is_symmetric = src.is_symmetric()
    if not is_symmetric:
        src = src.to_symmetric()
    if not src.storage.col().is_cuda or not src.is_quadratic():
        import scipy.sparse as sp
        sp_src = src.to_scipy(layout='csr')
        perm = sp.csgraph.reverse_cuthill_mckee(sp_src, symmetric_mode=True).copy()
        perm = torch.from_numpy(perm).to(torch.long).to(src.device())
        return permute(src, perm), perm
    rowptr, col, _ = src.csr()
    n = rowptr.numel() - 1
    deg = torch.ops.tsamd.rcm_degree(rowptr, col)
    if seeds == 'scipy':
        seed_order = _scipy_seed_order(deg, col.numel())
    else:
        ids = torch.arange(n, dtype=torch.long, device=col.device)
        seed_order = torch.ops.tsamd.sort_coo(deg, ids, col.numel() + 2, max(n, 1), True)[1]
    perm, _ = torch.ops.tsamd.rcm(rowptr, col, seed_order, -1)
    return permute(src, perm), perm


SparseTensor.reverse_cuthill_mckee = reverse_cuthill_mckee
