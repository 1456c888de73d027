"""tests/gat_attention_reference.py against itself and against torch on the CPU: the oracle against dense masked fp64
additive attention and its autograd (all four gradients), the float32 chain inside the derived bound on every test
layout, every planted defect of the restatement outside it, the census of every operand set the GPU tests use, and what
of the additive entry points needs no device: the status codes, case for case those of the dot-product call."""
import ctypes

import numpy as np
import pytest
import torch

from pytorch_sparse_amd import _native as nat
from tests import fused_attention_reference as F
from tests import gat_attention_reference as G

H, D, DTYPE = 2, 4, 'f32'  # the restatement's shape: chunks of 16 entries
SLOPE = 0.2


@pytest.fixture(scope='module')
def cases():
    r, census = G.layouts(DTYPE, H, D)
    assert r.chunk == 16
    sizes = F.edge_sizes(r.chunk, r.chunk, r.tile // 4, r.tile)
    return r, [F.edge_case(E) for E in sizes if E <= 2 * r.chunk + 1 or E >= r.tile - 1] + census


def _numbers(ops, dtype=DTYPE):
    return G.Operands(*[G.numbers(a, dtype) for a in ops])


def _dense(mask, row, col, a_dst, a_src, v, slope, bias=None):
    """Dense masked additive attention in torch -> (out, lse)."""
    z = a_dst[:, None, :] + a_src[None, :, :]
    if bias is not None:
        b = bias if bias.dim() == 2 else bias[:, None].expand(-1, a_dst.size(1))
        z = z + torch.zeros_like(z).index_put((torch.from_numpy(row), torch.from_numpy(col)), b)
    s = torch.nn.functional.leaky_relu(z, slope)
    m3 = torch.from_numpy(mask)[:, :, None].expand_as(s)
    masked = torch.where(m3, s, torch.full_like(s, -np.inf))
    P = torch.softmax(masked, 1)
    P = torch.where(m3 & ~torch.isnan(P), P, torch.zeros_like(P))
    return torch.einsum('mnh,nhd->mhd', P, v), torch.logsumexp(masked, 1)


@pytest.mark.parametrize('slope', [0.2, 0.0, 1.0, -0.5])
def test_oracle_against_dense_masked_fp64_torch_and_autograd(slope):
    rng = np.random.default_rng(1)
    mask = rng.random((23, 17)) < 0.3
    mask[5] = False
    mask[:, 3] = False
    mask[11] = True
    row, col = np.nonzero(mask)
    ptr = np.zeros(24, np.int64)
    np.cumsum(np.bincount(row, minlength=23), out=ptr[1:])
    Hh, Dd = 3, 5
    a_dst, a_src, v, b1, b2 = G.gradcheck_operands(ptr, col, 23, 17, Hh, Dd, seed=2)
    go = rng.standard_normal((23, Hh, Dd))
    for bias in (None, b1, b2):
        leaves = [torch.from_numpy(a).clone().requires_grad_() for a in (a_dst, a_src, v)]
        tb = None if bias is None else torch.from_numpy(bias).clone().requires_grad_()
        want, want_lse = _dense(mask, row, col, leaves[0], leaves[1], leaves[2], slope, tb)
        ex = G.exact(ptr, col, bias, a_dst, a_src, v, slope)
        assert np.allclose(ex.out, want.detach().numpy(), rtol=1e-12, atol=1e-14)
        assert np.allclose(ex.lse, want_lse.detach().numpy(), rtol=1e-12, atol=1e-14)
        assert bool((ex.out[5] == 0).all()) and bool(np.isneginf(ex.lse[5]).all())
        grads = torch.autograd.grad(want, leaves + ([tb] if tb is not None else []), torch.from_numpy(go))
        got, _ = G.grads_exact(ptr, col, bias, a_dst, a_src, v, slope, go)
        for g, ref in zip(got[:3], grads):
            assert np.allclose(g, ref.numpy(), rtol=1e-11, atol=1e-13)
        if tb is not None:
            assert np.allclose(got.bias if tb.dim() == 2 else got.bias.sum(1), grads[3].numpy(), rtol=1e-11, atol=1e-13)
        p, dz, _, _ = G.bw_exact(ptr, col, bias, a_dst, a_src, v, ex.out, ex.lse, go, slope, 'f64')
        assert np.allclose(p, ex.p, rtol=1e-12, atol=1e-15) and np.allclose(dz, got.bias, rtol=0, atol=0)


def test_derivative_at_zero_is_the_slope_as_torch_has_it():
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z, 0.2).sum().backward()
    assert bool((z.grad == 0.2).all())
    ptr, ind = np.array([0, 2], np.int64), np.array([0, 1], np.int64)
    a_dst, a_src, v = np.array([[1.5]]), np.array([[-1.5], [0.25]]), np.array([[[1.0]], [[3.0]]])
    ex = G.exact(ptr, ind, None, a_dst, a_src, v, 0.2)
    assert ex.z[0, 0] == 0 and ex.z[1, 0] == 1.75
    p, dz, _, _ = G.bw_exact(ptr, ind, None, a_dst, a_src, v, ex.out, ex.lse, np.ones((1, 1, 1)), 0.2, 'f64')
    ds0 = p[0, 0] * (1.0 - ex.out[0, 0, 0])
    assert ds0 != 0 and dz[0, 0] == ds0 * 0.2


def test_oracle_non_finite_rules_and_the_minus_inf_bias():
    ptr = np.array([0, 2, 4, 6, 6, 7], np.int64)
    ind = np.array([0, 1, 0, 1, 0, 1, 1], np.int64)
    a_dst, a_src, v = np.ones((5, 1)), np.ones((2, 1)), np.arange(4.0).reshape(2, 1, 2)
    bias = np.array([0.0, -np.inf, -np.inf, -np.inf, np.inf, 0.0, np.nan])
    ex = G.exact(ptr, ind, bias, a_dst, a_src, v, 0.2)
    assert np.array_equal(ex.out[0, 0], v[0, 0]), '-inf beside a finite score weighs zero'
    assert np.isnan(ex.out[1]).all() and np.isneginf(ex.lse[1, 0]), 'a row of -inf only'
    assert np.isnan(ex.out[2]).all() and np.isnan(ex.lse[2, 0]), '+inf'
    assert bool((ex.out[3] == 0).all()) and np.isneginf(ex.lse[3, 0]), 'no entries'
    assert np.isnan(ex.out[4]).all() and np.isnan(ex.lse[4, 0]), 'NaN'
    got = G.emulate(ptr, ind, bias, a_dst, a_src, v, 0.2, 4, 'f32')
    G.check(got[0], got[1], ex, 'f32')
    p, dz, _, _ = G.bw_exact(ptr, ind, bias, a_dst, a_src, v, ex.out, ex.lse, np.ones((5, 1, 2)), 0.2, 'f32')
    assert p[1, 0] == 0 and dz[1, 0] == 0 and np.isnan(p[2:4]).all() and np.isnan(dz[4:]).all()
    zero = G.exact(ptr, ind, bias, a_dst, a_src, v, 0.0)  # slope 0: 0 * -inf is NaN, the mask is lost
    assert np.isnan(zero.out[0]).all() and np.isnan(zero.lse[1, 0])
    t = torch.nn.functional.leaky_relu(torch.tensor([-np.inf]), 0.0)
    assert bool(torch.isnan(t).all()), 'torch has the same product'


@pytest.mark.parametrize('spread', [1.0, 40.0], ids=['ordinary', 'scores_pm80'])
def test_float32_chain_and_the_restatement_inside_the_bound(cases, spread):
    r, layouts = cases
    worst_c = worst_e = top = 0.0
    for i, case in enumerate(layouts):
        slope = (0.2, 0.0, 1.0)[i % 3]
        o = _numbers(G.operands(case, DTYPE, H, D, seed=11 + i, form=i % 3, spread=spread))
        ex = G.exact(case.ptr, case.ind, o.bias, o.a_dst, o.a_src, o.v, slope)
        top = max(top, float(np.abs(ex.s).max()))
        worst_c = max(worst_c, *G.check(*G.composition_f32(case.ptr, case.ind, o.bias, o.a_dst, o.a_src, o.v, slope),
                                        ex, DTYPE))
        if case.E <= 2 * r.chunk + 1 or case.name in ('hub', 'one_source'):
            worst_e = max(worst_e, *G.check(*G.emulate(case.ptr, case.ind, o.bias, o.a_dst, o.a_src, o.v, slope, r.chunk,
                                                       DTYPE), ex, DTYPE))
    assert spread == 1.0 or top > 80, 'an unshifted fp32 exp overflows (above 88.7) or flushes at such scores'
    print('float32 chain: worst err / bound %.3g; restatement %.3g' % (worst_c, worst_e))


@pytest.mark.parametrize('where', G.PEAKS)
def test_hub_with_the_maximum_in_its_first_chunk_its_last_and_both(cases, where):
    r, layouts = cases
    hub = layouts[-3]
    assert hub.name == 'hub'
    o = _numbers(G.operands(hub, DTYPE, H, D, seed=21, bias=F.peak_bias(hub, r.chunk, where, height=25.0)))
    ex = G.exact(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE)
    h = int(np.argmax(np.diff(hub.ptr)))
    lo, hi = int(hub.ptr[h]), int(hub.ptr[h + 1])
    top = np.argmax(ex.s[lo:hi], 0) + lo
    want = {'first': [lo + 1], 'last': [hi - 2], 'both': [lo + 1]}[where]
    assert set(top.tolist()) <= set(want), 'the planted peak is the maximum of the hub row in every head'
    G.check(*G.composition_f32(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE), ex, DTYPE)
    G.check(*G.emulate(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE, r.chunk, DTYPE), ex, DTYPE)


@pytest.mark.parametrize('mutant', G.SCORE_MUTANTS)
def test_every_planted_score_defect_is_rejected(cases, mutant):
    r, layouts = cases
    hub = layouts[-3]
    o = _numbers(G.operands(hub, DTYPE, H, D, seed=31, form=1))
    ex = G.exact(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE)
    G.check(*G.emulate(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE, r.chunk, DTYPE), ex, DTYPE)
    out, lse = G.emulate(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE, r.chunk, DTYPE, mutant=mutant)
    assert G.rejects(G.check, out, lse, ex, DTYPE), mutant


@pytest.mark.parametrize('mutant', G.GRAD_MUTANTS)
def test_every_planted_gradient_defect_is_rejected(cases, mutant):
    r, layouts = cases
    hub = layouts[-3]
    o = _numbers(G.operands(hub, DTYPE, H, D, seed=41, form=2))
    ex = G.exact(hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v, SLOPE)
    out, lse = F.numbers(F.store(ex.out, DTYPE), DTYPE), ex.lse.astype(np.float32).astype(np.float64)
    go = F.numbers(F.store(np.random.default_rng(42).standard_normal(ex.out.shape), DTYPE), DTYPE)
    args = (hub.ptr, hub.ind, o.bias, o.a_dst, o.a_src, o.v)
    expect_bw = G.bw_exact(*args, out, lse, go, SLOPE, DTYPE)
    expect = G.grads_exact(*args, SLOPE, go, DTYPE, out, lse)
    p, dz, grads = G.emulate_grads(*args, out, lse, go, SLOPE, DTYPE)
    G.check_bw(p, dz, expect_bw, DTYPE)
    G.check_grads(grads, expect, DTYPE)
    G.check_grads(grads._replace(bias=F.store(F.numbers(dz, DTYPE).sum(1), DTYPE)), expect, DTYPE, shared_bias=True)
    p, dz, grads = G.emulate_grads(*args, out, lse, go, SLOPE, DTYPE, mutant=mutant)
    if mutant == 'grad_a_src_by_rows':
        G.check_bw(p, dz, expect_bw, DTYPE)
    else:
        assert G.rejects(G.check_bw, p, dz, expect_bw, DTYPE), mutant
    assert G.rejects(G.check_grads, grads, expect, DTYPE), mutant


def test_census_of_every_operand_set_of_the_gpu_tests():
    """At least a quarter of the (entry, head) pairs on either side of the kink and one exactly on it, for every set; the
    layouts' own censuses (fused_attention_reference.layouts) are asserted as each is built."""
    sets = G.gpu_sets()
    assert len(sets) > 150 and {s.kind for s in sets} >= {'shape', 'wide', 'layout', 'peak', 'large', 'backward', 'public'}
    for s in sets:
        r, case, ops = G.build(s)
        c = G.census(case.ptr, case.ind, ops, s.dtype)
        assert c['neg'] >= 0.25 and c['pos'] >= 0.25 and c['zero'] >= 1, (s, c)
        assert case.E <= 2048 + 600, (s, case.E)
        if s.kind == 'large':
            z, _ = G.preact(case.ptr, case.ind, None, G.numbers(ops.a_dst, s.dtype), G.numbers(ops.a_src, s.dtype))
            assert float(z.max()) > 80 and float(z.min()) < -80


def test_gradcheck_operands_stay_off_the_kink():
    rng = np.random.default_rng(160)
    mask = rng.random((12, 9)) < 0.35
    row, col = np.nonzero(mask)
    ptr = np.zeros(13, np.int64)
    np.cumsum(np.bincount(row, minlength=12), out=ptr[1:])
    a_dst, a_src, v, b1, b2 = G.gradcheck_operands(ptr, col, 12, 9, 2, 3, seed=160)
    for b in (None, b1, b2):
        assert float(np.abs(G.preact(ptr, col, b, a_dst, a_src)[0]).min()) >= 1e-2


# ---- the additive entry points without a device ---------------------------------------------------------------------
def test_route_and_workspace_serve_the_additive_call():
    """The lane map is that of the dot-product call; the packet route looks at v and out alone (NULL counts as aligned)."""
    L = nat.lib()
    for dtype in G.FLOATS:
        for Hh, Dd in ((1, 1), (8, 16), (3, 5), (2, 300)):
            for aligned in (True, False):
                out = (ctypes.c_int64 * 8)()
                f = F.AR._fake(aligned)
                assert L.tsamd_attention_heads_route(F.CODE[dtype], Hh, Dd, None, None, f, f, out) == 0
                assert F.AtRoute(*[int(x) for x in out]) == F.expected_route(dtype, Hh, Dd, aligned)


def test_status_codes_decided_on_the_host():
    L = nat.lib()
    OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
    fake, sz = ctypes.c_void_p(0x1000), ctypes.c_size_t

    def fw(dtype=0, ptr=fake, col=fake, bias=None, bh=1, a_dst=fake, a_src=fake, v=fake, out=fake, lse=fake, M=4, N=4,
           Hh=2, Dd=3, E=5, ws=fake, nbytes=1 << 30):
        return L.tsamd_gat_attention_heads(dtype, ptr, col, bias, bh, a_dst, a_src, v, 0.2, out, lse, M, N, Hh, Dd, E, ws,
                                           sz(nbytes), None)

    def bw(dtype=0, row=None, ptr=fake, col=fake, bias=None, bh=1, a_dst=fake, a_src=fake, v=fake, out=fake, lse=fake,
           go=fake, p=fake, dz=fake, M=4, N=4, Hh=2, Dd=3, E=5):
        return L.tsamd_gat_attention_heads_bw(dtype, row, ptr, col, bias, bh, a_dst, a_src, v, out, lse, go, 0.2, p, dz, M,
                                              N, Hh, Dd, E, None)

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
    for null in ('ptr', 'col', 'a_dst', 'a_src', 'v'):
        assert fw(**{null: None}) == INVALID, null
    assert fw(N=0) == INVALID
    assert fw(ws=None) == WORKSPACE and fw(nbytes=F.workspace_bytes('f32', 2, 3, 5) - 1) == WORKSPACE
    assert bw(E=0) == OK and bw(Hh=0) == OK
    assert bw(Dd=0) == INVALID and bw(M=0) == INVALID and bw(N=0) == INVALID
    for null in ('col', 'a_dst', 'a_src', 'v', 'out', 'lse', 'go', 'p', 'dz'):
        assert bw(**{null: None}) == INVALID, null
    assert bw(ptr=None) == INVALID, 'row and rowptr both null'
