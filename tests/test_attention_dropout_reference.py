"""Dropout on the probabilities of the fused attention calls, on the CPU: the library's mask query against the numpy
restatement word for word, its status codes, the law of the mask, the oracle of tests/attention_dropout_reference.py
against dense masked fp64 torch and its autograd, the float32 chain inside the bound, and the comparators against planted
defects.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import np_draws as npd
from pytorch_sparse_amd import _native as nat
from tests import attention_dropout_reference as R
from tests import fused_attention_reference as F
from tests import gat_attention_reference as G

RATES = (0.0, 2.0 ** -32, 0.1, 0.5, 0.6, 1.0 - 2.0 ** -20)
SEEDS = (0, 1, 2 ** 63 - 1)


def query(seed, rate, e0, n, H):
    keep = np.full((n, H), 7, np.uint8)
    st = nat.lib().tsamd_attention_dropout_mask(seed, rate, e0, n, H, keep.ctypes.data_as(ctypes.c_void_p))
    assert st == 0, st
    assert set(np.unique(keep)) <= {0, 1}
    return keep.astype(bool)


# ---- 1, 2: the query ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', RATES)
def test_mask_query_equals_the_numpy_restatement(rate):
    """Fails without the feature: the symbol does not exist.  Ties the rule the kernels compile to oracle/np_draws.philox."""
    for seed in SEEDS:
        for e0 in (0, 1, 2, 3, 2 ** 32 - 2):
            for H in (1, 3, 64):
                got = query(seed, rate, e0, 9, H)
                assert np.array_equal(got, R.keep_mask(seed, rate, 9, H, e0)), (seed, rate, e0, H)
    if rate == 0.0:
        assert got.all()
    if rate == 2.0 ** -32:
        assert R.threshold(rate) == 1
    if rate == 1.0 - 2.0 ** -20:
        assert R.threshold(rate) == 2 ** 32 - 2 ** 12


def test_mask_query_status_codes():
    L = nat.lib()
    keep = np.zeros((4, 2), np.uint8)
    p = keep.ctypes.data_as(ctypes.c_void_p)
    invalid = 1
    assert L.tsamd_status_string(invalid).decode().lower().find('invalid') >= 0
    assert L.tsamd_attention_dropout_mask(0, 0.5, 0, 4, 2, None) == invalid
    assert L.tsamd_attention_dropout_mask(0, 0.5, 0, -1, 2, p) == invalid
    assert L.tsamd_attention_dropout_mask(0, 0.5, 0, 4, -1, p) == invalid
    assert L.tsamd_attention_dropout_mask(0, 0.5, -1, 4, 2, p) == invalid
    for rate in (1.0, 1.5, -0.1, -2.0 ** -40, float('nan'), float('inf'), float('-inf')):
        assert L.tsamd_attention_dropout_mask(0, rate, 0, 4, 2, p) == invalid, rate
    assert not keep.any(), 'a refused call writes nothing'
    assert L.tsamd_attention_dropout_mask(0, 0.5, 0, 0, 2, p) == 0 and L.tsamd_attention_dropout_mask(0, 0.5, 0, 4, 0, p) == 0
    assert L.tsamd_attention_dropout_mask(0, math.nextafter(1.0, 0.0), 0, 4, 2, p) == 0


# ---- 3: the law -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', [0.1, 0.5, 0.6])
def test_kept_share_is_binomial(rate):
    """2^18 (entry, head) pairs, kept / dropped against (1 - q, q) with q = thr / 2^32: the two-sided chi-square bound of
    tests/test_draw_oracle.py, |chi2 - dof| <= 5 sqrt(2 dof) + 5 with dof = 1."""
    E, H = 2 ** 14, 16
    keep = R.keep_mask(12345, rate, E, H)
    q = R.threshold(rate) / 2.0 ** 32
    n = E * H
    counts = np.array([keep.sum(), n - keep.sum()], np.float64)
    expected = np.array([n * (1 - q), n * q])
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print('rate %.1f: kept %.5f of %d, chi2 %.2f' % (rate, counts[0] / n, n, chi2))
    assert abs(chi2 - 1) <= 5 * math.sqrt(2) + 5
    # per head and per word of a batch as well: no head and no word is special
    for part in ([keep[:, h] for h in range(H)], [keep[w::4] for w in range(4)]):
        for k in part:
            exp = np.array([k.size * (1 - q), k.size * q])
            c2 = float(((np.array([k.sum(), k.size - k.sum()]) - exp) ** 2 / exp).sum())
            assert abs(c2 - 1) <= 5 * math.sqrt(2) + 5


def test_mask_depends_on_seed_and_head_and_rate_zero_keeps_everything():
    a = R.keep_mask(5, 0.5, 4096, 4)
    assert not np.array_equal(a, R.keep_mask(6, 0.5, 4096, 4))
    assert not np.array_equal(a, R.keep_mask(5 + 2 ** 32, 0.5, 4096, 4)), 'the high word of the seed is part of the key'
    for h in range(1, 4):
        assert not np.array_equal(a[:, 0], a[:, h])
        assert abs(float((a[:, 0] == a[:, h]).mean()) - 0.5) < 0.05
    assert R.keep_mask(5, 0.0, 4096, 4).all()
    # the entries of [e0, e0 + n) are those of the whole range: a pure function of the entry
    assert np.array_equal(R.keep_mask(5, 0.5, 100, 4, e0=37), a[37:137])
    # a lower rate keeps a superset
    assert bool((R.keep_mask(5, 0.1, 4096, 4) | ~a).all())


def test_host_seed_rule_is_the_samplers():
    import importlib
    att = importlib.import_module('pytorch_sparse_amd.attention')  # the package exports the function of that name
    torch.manual_seed(3)
    s = att._host_seed()
    assert s == npd.host_seed(3) and 0 <= s < 2 ** 63
    assert att._host_seed() != s


# ---- 4: the oracle against dense masked fp64 torch --------------------------------------------------------------------
def _small(seed=0, M=40, N=30):
    rng = np.random.default_rng(seed)
    mask = rng.random((M, N)) < 0.2
    mask[5] = True
    mask[7:10] = False
    mask[:, 11] = False
    row, col = np.nonzero(mask)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=M))]).astype(np.int64)
    return mask, row.astype(np.int64), col.astype(np.int64), ptr


def _operands(mode, rng, M, N, H, D, E, form):
    sr = rng.standard_normal((M, H, D) if mode == 'dot' else (M, H))
    sc = rng.standard_normal((N, H, D) if mode == 'dot' else (N, H))
    v = rng.standard_normal((N, H, D))
    bias = (None, rng.standard_normal(E), rng.standard_normal((E, H)))[form]
    return sr, sc, v, bias


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('form', [0, 1, 2])
def test_oracle_equals_dense_masked_torch_and_its_autograd(mode, form):
    mask, row, col, ptr = _small()
    M, N = mask.shape
    H, D, E = 3, 4, row.size
    rng = np.random.default_rng(10 + form)
    sr, sc, v, bias = _operands(mode, rng, M, N, H, D, E, form)
    scalar = 0.6 if mode == 'dot' else 0.2
    rate, seed = 0.6, 99
    keep, c = R.keep_mask(seed, rate, E, H), R.scale_of(rate)
    assert 0.3 < keep.mean() < 0.5
    ex = R.exact_dropout(R.plain_exact(mode, ptr, col, bias, sr, sc, v, scalar), ptr, col, v, keep, c)
    leaves = [torch.from_numpy(a).requires_grad_() for a in (sr, sc, v)]
    tb = None if bias is None else torch.from_numpy(bias).requires_grad_()
    want = R.dense_torch(mode, mask, row, col, tb, leaves[0], leaves[1], leaves[2], scalar, keep, c)
    assert np.allclose(ex.out, want.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert bool((ex.out[7:10] == 0).all())
    go = rng.standard_normal((M, H, D))
    grads = torch.autograd.grad(want, leaves + ([tb] if form else []), torch.from_numpy(go))
    ref, _ = R.grads_exact(mode, ptr, col, bias, sr, sc, v, scalar, go, keep, c)
    for g, w, name in zip(grads[:3], ref[:3], ('sr', 'sc', 'v')):
        assert np.allclose(g.numpy(), w, rtol=1e-11, atol=1e-13), name
    if form:
        wb = ref.bias if form == 2 else ref.bias.sum(1)
        assert np.allclose(grads[3].numpy(), wb, rtol=1e-11, atol=1e-13)
    # the plain oracle is the rate-0 case
    ex0 = R.plain_exact(mode, ptr, col, bias, sr, sc, v, scalar)
    same = R.exact_dropout(ex0, ptr, col, v, np.ones((E, H), bool), 1.0)
    for f in ('out', 'pav', 'a1', 'a2'):
        assert np.allclose(getattr(same, f), getattr(ex0, f), rtol=1e-13, atol=0), f


# ---- 5, 6: the bound, and what it rejects -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hub():
    """f32, H = 2, D = 3: a group of two lanes (per-entry Philox in the kernel), chunks of 16 entries."""
    H, D = 2, 3
    r, cases = F.layouts('f32', H, D)
    assert r.lanes_per_head * r.heads_per_pass == 2 and r.chunk == 16
    return r, cases[0], H, D


def _hub_operands(mode, case, H, D, seed):
    if mode == 'dot':
        q, k, v = F.operands(case, 'f32', H, D, seed=seed)
        return q, k, v, F.store(np.random.default_rng(seed + 1).standard_normal((case.E, H)), 'f32'), D ** -0.5
    ops = G.operands(case, 'f32', H, D, seed=seed, form=2)
    return ops.a_dst, ops.a_src, ops.v, ops.bias, 0.2


@pytest.mark.parametrize('mode', R.MODES)
def test_float32_chain_and_the_restated_kernel_stay_inside_the_bound(mode, hub):
    r, case, H, D = hub
    sr, sc, v, bias, scalar = _hub_operands(mode, case, H, D, 20)
    for rate, seed in ((0.1, 1), (0.6, 2)):
        keep, c = R.keep_mask(seed, rate, case.E, H), R.scale_of(rate)
        ex = R.exact_dropout(R.plain_exact(mode, case.ptr, case.ind, bias, sr, sc, v, scalar), case.ptr, case.ind, v, keep, c)
        out, lse = R.composition_f32(mode, case.ptr, case.ind, bias, sr, sc, v, scalar, keep, c)
        ra = R.check(mode, out, lse, ex, 'f32')
        out, lse = R.emulate(mode, case.ptr, case.ind, bias, sr, sc, v, scalar, r.chunk, 'f32', seed, rate)
        rb = R.check(mode, out, lse, ex, 'f32')
        print('%s rate %.1f: worst err / bound, chain out %.3g lse %.3g, restated kernel out %.3g lse %.3g'
              % ((mode, rate) + ra + rb))


@pytest.mark.parametrize('mode', R.MODES)
def test_comparator_rejects_planted_forward_defects(mode, hub):
    r, case, H, D = hub
    sr, sc, v, bias, scalar = _hub_operands(mode, case, H, D, 30)
    rate, seed = 0.5, 7
    keep, c = R.keep_mask(seed, rate, case.E, H), R.scale_of(rate)
    ex = R.exact_dropout(R.plain_exact(mode, case.ptr, case.ind, bias, sr, sc, v, scalar), case.ptr, case.ind, v, keep, c)
    R.check(mode, *R.emulate(mode, case.ptr, case.ind, bias, sr, sc, v, scalar, r.chunk, 'f32', seed, rate), ex, 'f32')
    for mutant in R.FW_MUTANTS:
        out, lse = R.emulate(mode, case.ptr, case.ind, bias, sr, sc, v, scalar, r.chunk, 'f32', seed, rate, mutant=mutant,
                             lpr=r.lanes_per_head * r.heads_per_pass)
        assert R.rejects(R.check, mode, out, lse, ex, 'f32'), mutant
    # the batch rule with a group as wide as a batch is the rule itself: aligned to e either way
    assert np.array_equal(R.keep_mask_by_window(seed, rate, case.E, H, 4), keep)
    assert not np.array_equal(R.keep_mask_by_window(seed, rate, case.E, H, 2), keep)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_comparator_rejects_planted_backward_defects(mode, dtype):
    case = F.edge_case(64 * 2 + 9, nsrc=23)
    H, D = 3, 8
    if mode == 'dot':
        q, k, v = F.operands(case, dtype, H, D, seed=40)
        sr, sc, bias, scalar = q, k, F.store(np.random.default_rng(41).standard_normal(case.E), dtype), 0.1 * D ** -0.5
    else:
        ops = G.operands(case, dtype, H, D, seed=40, form=1)
        sr, sc, v, bias, scalar = ops.a_dst, ops.a_src, ops.v, ops.bias, 0.2
    n = [F.numbers(a, dtype) for a in (sr, sc, v, bias)]
    rate, seed = 0.6, 11
    keep, c = R.keep_mask(seed, rate, case.E, H), R.scale_of(rate)
    ex = R.exact_dropout(R.plain_exact(mode, case.ptr, case.ind, n[3], n[0], n[1], n[2], scalar), case.ptr, case.ind, n[2], keep, c)
    out, lse = F.store(ex.out, dtype), ex.lse.astype(F.ACC[dtype])
    go = F.store(np.random.default_rng(42).standard_normal(ex.out.shape), dtype)
    no, ng = F.numbers(out, dtype), F.numbers(go, dtype)
    expect = R.bw_exact(mode, case.ptr, case.ind, n[3], n[0], n[1], n[2], no, lse.astype(np.float64), ng, scalar, keep, c, dtype)
    assert np.array_equal(expect[0] != 0, keep), 'every kept pt is above zero in the oracle'
    got = R.emulate_bw(mode, case.ptr, case.ind, n[3], n[0], n[1], n[2], no, lse, ng, scalar, dtype, seed, rate)
    w = R.check_bw(got[0], got[1], expect, dtype)
    assert np.array_equal(F.numbers(got[0], dtype) != 0, keep)
    print('%s %s restated backward: worst err / bound pt %.3g d %.3g' % ((mode, dtype) + w))
    for mutant in R.BW_MUTANTS:
        got = R.emulate_bw(mode, case.ptr, case.ind, n[3], n[0], n[1], n[2], no, lse, ng, scalar, dtype, seed, rate, mutant)
        assert R.rejects(R.check_bw, got[0], got[1], expect, dtype), mutant
    # the gradients: grad_v built from p in the place of pt, and d without keep c in front of dp, leave the bounds
    refs, bnds = R.grads_exact(mode, case.ptr, case.ind, n[3], n[0], n[1], n[2], scalar, ng, keep, c, dtype, out=no,
                               lse=lse.astype(np.float64))
    plain = R.grads_exact(mode, case.ptr, case.ind, n[3], n[0], n[1], n[2], scalar, ng, np.ones_like(keep), 1.0, dtype,
                          out=no, lse=lse.astype(np.float64))[0]
    ok = R.Grads(*(F.store(a, dtype) for a in (refs.sr, refs.sc, refs.v, refs.bias)))
    R.check_grads(ok, (refs, bnds), dtype)
    bad = R.Grads(*(F.store(a, dtype) for a in (plain.sr, plain.sc, plain.v, plain.bias)))
    for name in R.Grads._fields:
        one = R.Grads(*(getattr(bad if f == name else ok, f) for f in R.Grads._fields))
        assert R.rejects(R.check_grads, one, (refs, bnds), dtype), name
