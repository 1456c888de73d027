"""tests/fused_attention_reference.py against itself and against torch on the CPU: the oracle against dense masked fp64
attention and its autograd, the float32 three-step composition inside the derived bound on every test layout, every
planted defect of the restatement outside it, and what of csrc/attention.hip needs no device: the route pinned with
literals, the status codes and the workspace formula."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import fused_attention_reference as F

H, D, DTYPE = 2, 4, 'f32'  # the restatement's shape: chunks of 16 entries
ORDINARY = dict(scale=0.5, spread=1.0)
BIG = dict(scale=0.5, spread=40.0)  # scores of standard deviation 40: +-80 and beyond are met


def _cases():
    r, census = F.layouts(DTYPE, H, D)
    assert r.chunk == 16
    sizes = F.edge_sizes(r.chunk, r.chunk, r.tile // 4, r.tile)
    return r, [F.edge_case(E) for E in sizes if E <= 2 * r.chunk + 1 or E >= r.tile - 1] + census


@pytest.fixture(scope='module')
def cases():
    return _cases()


def _numbers(case, seed, spread, dtype=DTYPE):
    return tuple(F.numbers(a, dtype) for a in F.operands(case, dtype, H, D, seed=seed, spread=spread))


def test_oracle_against_dense_masked_fp64_attention_and_autograd():
    rng = np.random.default_rng(1)
    mask = rng.random((23, 17)) < 0.3
    mask[5] = False
    mask[:, 3] = False
    mask[11] = True
    row, col = np.nonzero(mask)
    ptr = np.zeros(24, np.int64)
    np.cumsum(np.bincount(row, minlength=23), out=ptr[1:])
    Hh, Dd = 3, 5
    q, k, v = (rng.standard_normal(s) for s in ((23, Hh, Dd), (17, Hh, Dd), (17, Hh, Dd)))
    go = rng.standard_normal((23, Hh, Dd))
    for bias in (None, rng.standard_normal(row.size), rng.standard_normal((row.size, Hh))):
        tq, tk, tv = (torch.from_numpy(a).clone().requires_grad_() for a in (q, k, v))
        scores = torch.einsum('mhd,nhd->mnh', tq, tk) * 0.7
        tb = None
        if bias is not None:
            tb = torch.from_numpy(bias).clone().requires_grad_()
            dense = torch.zeros(23, 17, Hh, dtype=torch.float64)
            idx = (torch.from_numpy(row), torch.from_numpy(col))
            scores = scores + dense.index_put(idx, tb if tb.dim() == 2 else tb[:, None].expand(-1, Hh))
        m3 = torch.from_numpy(mask)[:, :, None].expand_as(scores)
        masked = torch.where(m3, scores, torch.full_like(scores, -np.inf))
        P = torch.where(m3, torch.softmax(masked, 1), torch.zeros_like(scores))
        P = torch.where(torch.isnan(P), torch.zeros_like(P), P)  # rows without entries
        want = torch.einsum('mnh,nhd->mhd', P, tv)
        want_lse = torch.logsumexp(masked, 1)
        ex = F.exact(ptr, col, bias, q, k, v, 0.7)
        assert np.allclose(ex.out, want.detach().numpy(), rtol=1e-12, atol=1e-14)
        assert np.allclose(ex.lse, want_lse.detach().numpy(), rtol=1e-12, atol=1e-14)
        assert bool((ex.out[5] == 0).all()) and bool(np.isneginf(ex.lse[5]).all())
        grads = torch.autograd.grad(want, (tq, tk, tv) + ((tb, ) if tb is not None else ()), torch.from_numpy(go))
        gq, gk, gv, ds = F.grads_exact(ptr, col, bias, q, k, v, 0.7, go)
        for got, ref in zip((gq, gk, gv), grads):
            assert np.allclose(got, ref.numpy(), rtol=1e-11, atol=1e-13)
        if tb is not None:
            assert np.allclose(ds if tb.dim() == 2 else ds.sum(1), grads[3].numpy(), rtol=1e-11, atol=1e-13)
        # the backward kernel's two arrays from the oracle's own out and lse
        p, ds2, _, _ = F.bw_exact(ptr, col, bias, q, k, v, ex.out, ex.lse, go, 0.7)
        assert np.allclose(p, ex.p, rtol=1e-12, atol=1e-15) and np.allclose(ds2, ds, rtol=1e-10, atol=1e-14)


def test_oracle_non_finite_rules():
    ptr = np.array([0, 2, 4, 6, 6, 7], np.int64)
    ind = np.array([0, 1, 0, 1, 0, 1, 1], np.int64)
    q, k, v = np.ones((5, 1, 2)), np.ones((2, 1, 2)), np.arange(4.0).reshape(2, 1, 2)
    bias = np.array([0.0, -np.inf, -np.inf, -np.inf, np.inf, 0.0, np.nan])
    ex = F.exact(ptr, ind, bias, q, k, v, 1.0)
    assert np.array_equal(ex.out[0, 0], v[0, 0]), '-inf beside a finite score weighs zero'
    assert np.isnan(ex.out[1]).all() and np.isneginf(ex.lse[1, 0]), 'a row of -inf only'
    assert np.isnan(ex.out[2]).all() and np.isnan(ex.lse[2, 0]), '+inf'
    assert bool((ex.out[3] == 0).all()) and np.isneginf(ex.lse[3, 0]), 'no entries'
    assert np.isnan(ex.out[4]).all() and np.isnan(ex.lse[4, 0]), 'NaN'
    got = F.emulate(ptr, ind, bias, q, k, v, 1.0, 4, 'f32')
    F.check(got[0], got[1], ex, 'f32')


@pytest.mark.parametrize('cfg', [ORDINARY, BIG], ids=['ordinary', 'scores_pm80'])
def test_float32_composition_and_the_restatement_inside_the_bound(cases, cfg):
    r, layouts = cases
    worst_c = worst_e = top = 0.0
    for i, case in enumerate(layouts):
        q, k, v = _numbers(case, 11 + i, cfg['spread'])
        bias = (None, F.numbers(F.store(np.random.default_rng(i).standard_normal(case.E), DTYPE), DTYPE),
                F.numbers(F.store(np.random.default_rng(i).standard_normal((case.E, H)), DTYPE), DTYPE))[i % 3]
        ex = F.exact(case.ptr, case.ind, bias, q, k, v, cfg['scale'])
        top = max(top, float(np.abs(ex.s).max()))
        worst_c = max(worst_c, *F.check(*F.composition_f32(case.ptr, case.ind, bias, q, k, v, cfg['scale']), ex, DTYPE))
        if case.E <= 2 * r.chunk + 1 or case.name in ('hub', 'one_source'):
            worst_e = max(worst_e, *F.check(*F.emulate(case.ptr, case.ind, bias, q, k, v, cfg['scale'], r.chunk, DTYPE),
                                            ex, DTYPE))
    assert cfg is not BIG or top > 80, 'an unshifted fp32 exp overflows (above 88.7) or flushes at such scores'
    print('float32 composition: worst err / bound %.3g; restatement %.3g' % (worst_c, worst_e))


@pytest.mark.parametrize('where', F.PEAKS)
def test_hub_with_the_maximum_in_its_first_chunk_its_last_and_both(cases, where):
    r, layouts = cases
    hub = layouts[-3]
    assert hub.name == 'hub'
    q, k, v = _numbers(hub, 21, 1.0)
    bias = F.peak_bias(hub, r.chunk, where)
    ex = F.exact(hub.ptr, hub.ind, bias, q, k, v, 0.5)
    h = int(np.argmax(np.diff(hub.ptr)))
    lo, hi = int(hub.ptr[h]), int(hub.ptr[h + 1])
    top = np.argmax(ex.s[lo:hi], 0) + lo
    want = {'first': [lo + 1], 'last': [hi - 2], 'both': [lo + 1]}[where]
    assert set(top.tolist()) <= set(want), 'the planted peak is the maximum of the hub row in every head'
    F.check(*F.composition_f32(hub.ptr, hub.ind, bias, q, k, v, 0.5), ex, DTYPE)
    F.check(*F.emulate(hub.ptr, hub.ind, bias, q, k, v, 0.5, r.chunk, DTYPE), ex, DTYPE)


@pytest.mark.parametrize('mutant', F.MUTANTS)
def test_every_planted_defect_is_rejected(cases, mutant):
    r, layouts = cases
    hub = layouts[-3]
    cfg = BIG if mutant == 'max_shared_between_heads' else ORDINARY
    q, k, v = _numbers(hub, 31, cfg['spread'])
    bias = F.peak_bias(hub, r.chunk, 'last')
    ex = F.exact(hub.ptr, hub.ind, bias, q, k, v, cfg['scale'])
    F.check(*F.emulate(hub.ptr, hub.ind, bias, q, k, v, cfg['scale'], r.chunk, DTYPE), ex, DTYPE)
    out, lse = F.emulate(hub.ptr, hub.ind, bias, q, k, v, cfg['scale'], r.chunk, DTYPE, mutant=mutant)
    assert F.rejects(out, lse, ex, DTYPE), mutant


# ---- csrc/attention.hip without a device ------------------------------------------------------------------------------
def test_route_pinned():
    R = F.AtRoute
    assert F.route('f32', 8, 16) == R(0, 4, 4, 8, 1, 256, 2048, 1)
    assert F.route('bf16', 8, 16) == R(0, 8, 2, 8, 1, 128, 2048, 1)
    assert F.route('bf16', 8, 16, aligned=False) == R(1, 1, 2, 8, 1, 128, 2048, 1)
    assert F.route('f32', 8, 64) == R(0, 4, 16, 4, 2, 512, 2048, 1)
    assert F.route('f32', 3, 5) == R(1, 1, 2, 4, 1, 64, 2048, 1)
    assert F.route('f32', 1, 1) == R(1, 1, 1, 1, 1, 8, 2048, 1)
    assert F.route('f64', 2, 128) == R(0, 2, 64, 1, 2, 512, 2048, 1)
    assert F.route('f16', 3, 24) == R(0, 8, 4, 4, 1, 128, 2048, 1)
    assert F.route('f32', 2, 300) == R(0, 4, 64, 1, 4, 512, 2048, 2), 'a head wider than 64 lanes: two feature blocks'
    for dtype in F.FLOATS:
        for Hh in (1, 2, 3, 8, 70):
            for Dd in (1, 3, 4, 8, 16, 24, 64, 128, 300):
                for aligned in (True, False):
                    got = F.route(dtype, Hh, Dd, aligned)
                    assert got == F.expected_route(dtype, Hh, Dd, aligned), (dtype, Hh, Dd, aligned)
                    assert got.lanes_per_head * got.heads_per_pass <= 64
                    assert got[2:] == F.route(dtype, Hh, Dd, not aligned)[2:], 'the lane map ignores the pointers'


def test_workspace_formula():
    ws = nat.lib().tsamd_attention_heads_workspace_bytes
    for dtype in F.FLOATS:
        for Hh, Dd, E in ((1, 1, 1), (8, 16, 100000), (3, 5, 2049), (2, 300, 513), (8, 128, 0)):
            assert ws(F.CODE[dtype], Hh, Dd, E) == F.workspace_bytes(dtype, Hh, Dd, E), (dtype, Hh, Dd, E)
    assert ws(4, 2, 4, 10) == 0 and ws(0, -1, 4, 10) == 0 and ws(0, 2, 4, -1) == 0 and ws(0, 1 << 20, 1 << 20, 10) == 0


def test_status_codes_decided_on_the_host():
    L = nat.lib()
    OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
    assert L.tsamd_status_string(WORKSPACE).decode().lower().find('workspace') >= 0
    fake, sz = ctypes.c_void_p(0x1000), ctypes.c_size_t
    route8 = (ctypes.c_int64 * 8)()
    assert L.tsamd_attention_heads_route(0, 2, 4, fake, fake, fake, fake, None) == INVALID
    assert L.tsamd_attention_heads_route(0, -1, 4, fake, fake, fake, fake, route8) == INVALID
    assert L.tsamd_attention_heads_route(0, 2, -4, fake, fake, fake, fake, route8) == INVALID
    assert L.tsamd_attention_heads_route(5, 2, 4, fake, fake, fake, fake, route8) == UNSUPPORTED
    assert L.tsamd_attention_heads_route(0, 1 << 20, 1 << 20, fake, fake, fake, fake, route8) == UNSUPPORTED

    def fw(dtype=0, ptr=fake, col=fake, bias=None, bh=1, q=fake, k=fake, v=fake, out=fake, lse=fake, M=4, N=4, Hh=2, Dd=3,
           E=5, ws=fake, nbytes=1 << 30):
        return L.tsamd_attention_heads(dtype, ptr, col, bias, bh, q, k, v, 1.0, out, lse, M, N, Hh, Dd, E, ws, sz(nbytes),
                                       None)

    def bw(dtype=0, row=None, ptr=fake, col=fake, bias=None, bh=1, q=fake, out=fake, lse=fake, go=fake, p=fake, ds=fake,
           M=4, N=4, Hh=2, Dd=3, E=5):
        return L.tsamd_attention_heads_bw(dtype, row, ptr, col, bias, bh, q, fake, fake, out, lse, go, 1.0, p, ds, M, N,
                                          Hh, Dd, E, None)

    for f in (fw, bw):
        for neg in ('M', 'N', 'Hh', 'Dd', 'E'):
            assert f(**{neg: -1}) == INVALID, neg
        assert f(dtype=4) == UNSUPPORTED and f(dtype=5) == UNSUPPORTED
        assert f(dtype=4, M=-1) == INVALID, 'a negative size is reported first'
        assert f(Hh=1 << 20, Dd=1 << 20) == UNSUPPORTED and f(M=1 << 31) == UNSUPPORTED and f(N=1 << 31) == UNSUPPORTED
        assert f(Hh=65536 * 64, Dd=1) == UNSUPPORTED, 'more than 65535 column blocks'
        assert f(bias=fake, bh=3) == INVALID
    assert fw(M=0) == OK and fw(Hh=0) == OK and fw(Dd=0) == OK
    assert fw(out=None) == INVALID and fw(lse=None) == INVALID
    for null in ('ptr', 'col', 'q', 'k', 'v'):
        assert fw(**{null: None}) == INVALID, null
    assert fw(N=0) == INVALID
    assert fw(ws=None) == WORKSPACE and fw(nbytes=F.workspace_bytes('f32', 2, 3, 5) - 1) == WORKSPACE
    assert bw(E=0) == OK and bw(Hh=0) == OK
    assert bw(Dd=0) == INVALID and bw(M=0) == INVALID and bw(N=0) == INVALID
    for null in ('col', 'q', 'out', 'lse', 'go', 'p', 'ds'):
        assert bw(**{null: None}) == INVALID, null
    assert bw(ptr=None) == INVALID, 'row and rowptr both null'
