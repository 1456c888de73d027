"""tests/attention_reference.py pinned on the CPU: the oracles against dense fp64 torch and its autograd, float32 torch
inside the comparators, the planted defects rejected, the route census, and the status codes the five C entries
decide before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import attention_reference as R

H, D = 3, 5


@pytest.fixture(scope='module')
def small():
    """A 40 x 30 pattern with columns repeated across rows, empty rows and columns, and its operands in fp64."""
    rng = np.random.default_rng(21)
    mask = rng.random((40, 30)) < 0.2
    mask[3:6] = False
    mask[:, 10:13] = False
    mask[17] = True
    mask[17, 10:13] = False
    row, col = np.nonzero(mask)
    ptr = np.zeros(41, np.int64)
    np.cumsum(np.bincount(row, minlength=40), out=ptr[1:])
    case = R.Case('small', ptr, col.astype(np.int64), int(col.size), 40, 30)
    q, k, v = (rng.standard_normal(s) for s in ((40, H, D), (30, H, D), (case.E, H)))
    return mask, row, col, case, q, k, v


def _dense_scores(mask, row, col, q, k, scale):
    """(q @ k.T) per head, masked: torch tensors in, the stored entries [E, H] out."""
    s = torch.einsum('mhd,nhd->mnh', q, k) * scale
    return s[torch.from_numpy(row), torch.from_numpy(col)]


def _dense_matmul(mask, row, col, v, x):
    """A_h @ x_h with A dense [M, N, H]."""
    A = torch.zeros(mask.shape + (v.shape[1], ), dtype=v.dtype)
    A = A.index_put((torch.from_numpy(row), torch.from_numpy(col)), v)
    return torch.einsum('mnh,nhd->mhd', A, x)


def test_oracles_agree_with_dense_fp64_torch_and_autograd(small):
    mask, row, col, case, q, k, v = small
    tq, tk, tv = (torch.from_numpy(a).requires_grad_() for a in (q, k, v))
    scale = 0.37
    want = _dense_scores(mask, row, col, tq, tk, scale)
    got, mass, n = R.sddmm_exact(case.ptr, case.ind, None, q, k, scale)
    assert n == D and np.allclose(got, want.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert bool((mass >= np.abs(got) * (1 - 1e-12)).all())
    g = np.random.default_rng(22).standard_normal(got.shape)
    gq, gk = torch.autograd.grad(want, (tq, tk), torch.from_numpy(g))
    (eq, _, nq), (ek, _, nk) = R.sddmm_grads_exact(case.ptr, case.ind, q, k, scale, g)
    assert np.allclose(eq, gq.numpy(), rtol=1e-13, atol=1e-15) and np.allclose(ek, gk.numpy(), rtol=1e-13, atol=1e-15)
    assert int(nq[17, 0, 0]) == 2 * int(mask[17].sum()) + 1 and int(nk[11, 0, 0]) == 1

    want = _dense_matmul(mask, row, col, tv, tk)
    got, mass, n = R.spmm_exact(case.ptr, case.ind, None, v, k, case.nseg)
    assert np.allclose(got, want.detach().numpy(), rtol=1e-13, atol=1e-15)
    assert bool((got[3:6] == 0).all()) and int(n[17, 0, 0]) == 2 * int(mask[17].sum())
    go = np.random.default_rng(23).standard_normal(got.shape)
    gv, gx = torch.autograd.grad(want, (tv, tk), torch.from_numpy(go))
    (ev, _, nv), (ex, _, _) = R.spmm_grads_exact(case.ptr, case.ind, v, k, case.nseg, go)
    assert nv == D
    assert np.allclose(ev, gv.numpy(), rtol=1e-13, atol=1e-15) and np.allclose(ex, gx.numpy(), rtol=1e-13, atol=1e-15)


def test_oracles_through_perm_are_the_transposed_products(small):
    """The column order (colptr, row ids, csr2csc): the SpMM through perm is A^T @ x, the SDDMM through perm writes the
    scores of the transposed pattern back in storage order."""
    mask, row, col, case, q, k, v = small
    colptr, row_csc, csr2csc = R.csc_of(case)
    got, _, _ = R.spmm_exact(colptr, row_csc, csr2csc, v, q, case.nsrc)
    A = torch.zeros(mask.shape + (H, ), dtype=torch.float64)
    A = A.index_put((torch.from_numpy(row), torch.from_numpy(col)), torch.from_numpy(v))
    want = torch.einsum('mnh,mhd->nhd', A, torch.from_numpy(q))
    assert np.allclose(got, want.numpy(), rtol=1e-13, atol=1e-15) and bool((got[10:13] == 0).all())
    plain, _, _ = R.sddmm_exact(case.ptr, case.ind, None, q, k, 1.5)
    through, _, _ = R.sddmm_exact(colptr, row_csc, csr2csc, k, q, 1.5)
    assert np.allclose(plain, through, rtol=1e-14, atol=0)
    # the gradients are the two products on the other order
    g = np.random.default_rng(24).standard_normal(plain.shape)
    (eq, _, _), (ek, _, _) = R.sddmm_grads_exact(case.ptr, case.ind, q, k, 1.5, g)
    assert np.allclose(eq, 1.5 * R.spmm_exact(case.ptr, case.ind, None, g, k, case.nseg)[0], rtol=1e-13, atol=1e-15)
    assert np.allclose(ek, 1.5 * R.spmm_exact(colptr, row_csc, csr2csc, g, q, case.nsrc)[0], rtol=1e-13, atol=1e-15)


def test_float32_torch_of_the_compositions_is_inside_the_bounds(small):
    mask, row, col, case, q, k, v = small
    q32, k32, v32 = (a.astype(np.float32) for a in (q, k, v))
    tq, tk, tv = (torch.from_numpy(a) for a in (q32, k32, v32))
    scale = 0.37
    worst = {}
    got = (tq[row] * tk[col]).sum(-1) * np.float32(scale)
    worst['sddmm'] = R.check(got.numpy(), R.sddmm_exact(case.ptr, case.ind, None, q32, k32, scale), 'f32')
    got = _dense_matmul(mask, row, col, tv, tk)
    worst['spmm'] = R.check(got.numpy(), R.spmm_exact(case.ptr, case.ind, None, v32, k32, case.nseg), 'f32')
    g = np.random.default_rng(25).standard_normal((case.E, H)).astype(np.float32)
    go = np.random.default_rng(26).standard_normal((case.nseg, H, D)).astype(np.float32)
    tq.requires_grad_(), tk.requires_grad_()
    gq, gk = torch.autograd.grad((tq[row] * tk[col]).sum(-1) * np.float32(scale), (tq, tk), torch.from_numpy(g))
    eq, ek = R.sddmm_grads_exact(case.ptr, case.ind, q32, k32, scale, g)
    worst['grad_q'], worst['grad_k'] = R.check(gq.numpy(), eq, 'f32'), R.check(gk.numpy(), ek, 'f32')
    tv.requires_grad_()
    gv, gx = torch.autograd.grad(_dense_matmul(mask, row, col, tv, tk), (tv, tk), torch.from_numpy(go))
    ev, ex = R.spmm_grads_exact(case.ptr, case.ind, v32, k32, case.nseg, go)
    worst['grad_value'], worst['grad_x'] = R.check(gv.numpy(), ev, 'f32'), R.check(gx.numpy(), ex, 'f32')
    print('float32 torch, worst error / bound: ' + ', '.join('%s %.3g' % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize('dtype', R.FLOATS)
def test_emulation_without_defects_passes_and_every_planted_defect_is_rejected(dtype):
    """The restatements by pieces on the hub layout of an 8-entry chunk (the shape of hub_case, short enough for the
    Python loops): without a defect inside the comparators, with any one of them outside.  The defects of the chunk /
    record scheme need a cut row to show, which the row order has; through perm (the column order of the same pattern,
    short columns) the ones that concern perm, the memset and the heads must show as well."""
    rng = np.random.default_rng(27)
    L = 8
    case = R._case('mini', [0, 0, 1, 3 * L + 5, 0, 1] + R._short_rows(rng, L - 3 - (3 * L + 7) % L + L) + [7, 2, 0, 0],
                   19, rng)
    c = R.census(case, L, 2048, 2048)
    assert c['span3'] >= 1 and c['cut'] >= 1 and c['empty'] >= 5
    q, k, v = R.operands(case, dtype, H, 8, seed=28)
    nq, nk, nv = (R.numbers(a, dtype) for a in (q, k, v))
    colptr, row_csc, perm = R.csc_of(case)
    scale = 0.6
    sd = R.sddmm_route(dtype, H, 8)
    for ptr, ind, pm, a, b in ((case.ptr, case.ind, None, nq, nk), (colptr, row_csc, perm, nk, nq)):
        expect = R.sddmm_exact(ptr, ind, pm, a, b, scale)
        clean = R.emulate_sddmm(ptr, ind, pm, a, b, scale, sd.lanes_per_head, sd.vec)
        assert R.check(R.store(clean, dtype), expect, dtype) <= 1.0
        for m in R.SDDMM_MUTANTS:
            if m == 'perm_ignored' and pm is None:
                continue
            bad = R.emulate_sddmm(ptr, ind, pm, a, b, scale, sd.lanes_per_head, sd.vec, mutant=m)
            assert R.rejects(R.store(bad, dtype), expect, dtype), m
    for ptr, ind, pm, x, nseg in ((case.ptr, case.ind, None, nk, case.nseg), (colptr, row_csc, perm, nq, case.nsrc)):
        expect = R.spmm_exact(ptr, ind, pm, nv, x, nseg)
        clean = R.emulate_spmm(ptr, ind, pm, nv, x, nseg, L)
        assert R.check(R.store(clean, dtype), expect, dtype) <= 1.0
        for m in R.SPMM_MUTANTS:
            if pm is None and m == 'perm_on_ind':
                continue
            bad = R.emulate_spmm(ptr, ind, pm, nv, x, nseg, L, mutant=m)
            if pm is None or m in ('perm_on_ind', 'empty_not_zeroed', 'value_of_next_head'):
                assert R.rejects(R.store(bad, dtype), expect, dtype), (m, pm is not None)
    assert len(R.SDDMM_MUTANTS) + len(R.SPMM_MUTANTS) >= 6


def test_route_queries_and_the_census_of_every_layout():
    for dtype in R.FLOATS:
        vec = 16 // R.ITEM[dtype]
        for Hh in (1, 2, 3, 8):
            for Dd in (1, 3, 4, 8, 16, 24, 64, 128):
                for aligned in (True, False):
                    s, m = R.sddmm_route(dtype, Hh, Dd, aligned), R.spmm_route(dtype, Hh, Dd, aligned)
                    assert s.generic == R.expected_sddmm_route(dtype, Hh, Dd, aligned), (dtype, Hh, Dd, aligned)
                    assert m.generic == R.expected_spmm_route(dtype, Hh, Dd, aligned), (dtype, Hh, Dd, aligned)
                    assert s.vec == (1 if s.generic else vec) and m.vec == (1 if m.generic else vec)
                    per_head = Dd // s.vec
                    assert s.lanes_per_head == min(64, 1 << (per_head - 1).bit_length())
                    assert s.lanes_per_head * s.heads_per_pass * s.side_by_side == 64
                    assert s.heads_per_pass <= s.max_heads == 16 and (s.window, s.block) == (64, 256)
                    assert m.lanes_per_row * m.groups == 64 and m.chunk == 8 * m.lanes_per_row
                    assert m.blocks * m.lanes_per_row * m.vec >= Hh * Dd > (m.blocks - 1) * m.lanes_per_row * m.vec
                    # the chunk, hence the workspace, does not depend on the alignment
                    assert m.chunk == R.spmm_route(dtype, Hh, Dd, True).chunk
        R.assert_census(dtype, 3, 8)
    # both SDDMM routes and both SpMM routes are reached by the shapes the GPU tests use
    assert {R.sddmm_route('f32', 3, d).generic for d in (5, 16)} == {0, 1}
    assert R.sddmm_route('f32', 3, 24).generic == 1, '6 packets per head: not a power of two'
    assert R.sddmm_route('f32', 3, 16, aligned=False).generic == 1


def test_entry_status_codes_before_any_device_call():
    L = nat.lib()
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    fake = vp(0x1000)  # never dereferenced
    INVALID, UNSUPPORTED, WORKSPACE, OK = 1, 2, 4, 0
    route8 = (ctypes.c_int64 * 8)()

    def sddmm(dtype=0, nseg=3, nsrc=3, H=2, D=4, E=4, row=fake, ptr=fake, ind=fake, q=fake, k=fake, out=fake):
        return L.tsamd_sddmm_heads(dtype, row, ptr, ind, None, q, k, 1.0, out, nseg, nsrc, H, D, E, None)

    def spmm(dtype=0, nseg=3, nsrc=3, H=2, D=4, E=4, ptr=fake, ind=fake, x=fake, out=fake, ws=fake, nbytes=1 << 20):
        return L.tsamd_spmm_heads(dtype, ptr, ind, None, None, x, out, nseg, nsrc, H, D, E, ws, sz(nbytes), None)

    for call in (sddmm, spmm):
        for name in ('nseg', 'nsrc', 'H', 'D', 'E'):
            assert call(**{name: -1}) == INVALID, name
        for dt in (4, 5, 6, 7, 8, 9, -1):  # the integers, unknown codes
            assert call(dtype=dt) == UNSUPPORTED
        assert call(nseg=-1, dtype=5) == INVALID, 'a negative size wins over the dtype'
        assert call(nseg=1 << 31) == UNSUPPORTED and call(nsrc=1 << 31) == UNSUPPORTED
        assert call(H=1 << 20, D=1 << 20) == UNSUPPORTED
        assert call(H=0, dtype=5) == UNSUPPORTED, 'the dtype is checked before the empty call returns'
        assert call(H=0, out=None, ptr=None, ind=None) == OK and call(D=0, out=None, ptr=None, ind=None) == OK
        assert call(out=None) == INVALID and call(ind=None) == INVALID
    assert sddmm(E=0, out=None, ptr=None, ind=None, q=None, k=None) == OK
    assert sddmm(q=None) == INVALID and sddmm(k=None) == INVALID and sddmm(nseg=0) == INVALID
    assert sddmm(row=None, ptr=None) == INVALID, 'the segment of an entry needs row or ptr'
    assert spmm(nseg=0, E=0, out=None, ptr=None, ind=None, x=None, ws=None) == OK
    assert spmm(x=None) == INVALID and spmm(ptr=None) == INVALID and spmm(nsrc=0) == INVALID
    assert spmm(H=1 << 16, D=1 << 7) == UNSUPPORTED, 'more column blocks than a grid carries'
    assert spmm(ws=None) == WORKSPACE and spmm(nbytes=255) == WORKSPACE
    assert spmm(out=None, ws=None) == INVALID, 'a null pointer wins over the workspace'

    assert L.tsamd_sddmm_heads_route(0, 2, 4, fake, fake, None) == INVALID
    assert L.tsamd_spmm_heads_route(0, 2, 4, fake, fake, None) == INVALID
    assert L.tsamd_sddmm_heads_route(0, -1, 4, fake, fake, route8) == INVALID
    assert L.tsamd_spmm_heads_route(0, 2, -4, fake, fake, route8) == INVALID
    assert L.tsamd_sddmm_heads_route(5, 2, 4, fake, fake, route8) == UNSUPPORTED
    assert L.tsamd_spmm_heads_route(4, 2, 4, fake, fake, route8) == UNSUPPORTED

    ws = L.tsamd_spmm_heads_workspace_bytes
    a256 = lambda x: -(-x // 256) * 256  # noqa: E731
    for name, dt, acc in (('f32', 0, 4), ('f64', 1, 8), ('f16', 2, 4), ('bf16', 3, 4)):
        for Hh, Dd in ((1, 1), (3, 5), (8, 16), (8, 64)):
            chunk = R.spmm_route(name, Hh, Dd).chunk
            for E in (1, chunk, chunk + 1, 70_000):
                nch = -(-E // chunk)
                assert ws(dt, 9, Hh, Dd, E) == 2 * a256(acc * nch * Hh * Dd) + 2 * a256(8 * nch), (name, Hh, Dd, E)
    assert ws(5, 9, 2, 4, 100) == 0 and ws(42, 9, 2, 4, 100) == 0 and ws(0, 9, -2, 4, 100) == 0
