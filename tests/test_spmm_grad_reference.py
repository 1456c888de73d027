"""The fp64 reference of the sum / mean SpMM backward (tests/spmm_grad_reference.py) held to torch's own autograd of
the dense restatement and to the C oracle; its case builders held to the properties they claim; and the comparator
shown to reject six planted defects while it accepts a plain same-precision computation.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as oc
from pytorch_sparse_amd import synth
from tests import spmm_grad_reference as R
from tests.util import FLOAT_DTYPES, SUM_ATOL, SUM_TOL


def _graphs():
    return [('edge', R.edge_graph()), ('rand40x33', R.random_graph(40, 33, 300, 1)),
            ('rand7x90', R.random_graph(7, 90, 120, 2))]


@pytest.mark.parametrize('reduce', ['sum', 'mean'])
@pytest.mark.parametrize('batch', [(), (2, )])
@pytest.mark.parametrize('with_value', [True, False])
def test_formulas_against_dense_autograd(reduce, batch, with_value):
    """to_dense matrix (rows divided by deg for mean) @ x, .backward(g), all in fp64 by torch's autograd."""
    for name, G in _graphs():
        K, E = 5, G.col.numel()
        x = synth.features(G.N, K, seed=11, dtype=torch.float64, batch=batch)
        g = synth.features(G.M, K, seed=12, dtype=torch.float64, batch=batch)
        value = R.edge_values(E, torch.float64, 13) if with_value else None
        ref = R.reference(G.row, G.col, value, x, g, reduce, G.M)
        v = (value.clone() if with_value else torch.ones(E, dtype=torch.float64)).requires_grad_()
        xd = x.clone().requires_grad_()
        A = torch.sparse_coo_tensor(torch.stack([G.row, G.col]), v, (G.M, G.N)).to_dense()
        if reduce == 'mean':
            A = A / torch.bincount(G.row, minlength=G.M).clamp(min=1).double().view(-1, 1)
        out = A @ xd
        out.backward(g)
        scale = max(1.0, float(ref.out_l1.max()), float(ref.grad_mat_l1.max()), float(ref.grad_value_l1.max()))
        tol = 1e-13 * scale
        assert out.shape == ref.out.shape and xd.grad.shape == ref.grad_mat.shape, name
        assert float((out.detach() - ref.out).abs().max()) <= tol, name
        assert float((xd.grad - ref.grad_mat).abs().max()) <= tol, name
        assert float((v.grad - ref.grad_value).abs().max()) <= tol, name
        # the masses dominate the results and vanish exactly where nothing is summed
        assert bool((ref.out.abs() <= ref.out_l1 * (1 + 1e-12)).all())
        assert bool((ref.grad_mat.abs() <= ref.grad_mat_l1 * (1 + 1e-12)).all())
        assert bool((ref.grad_value.abs() <= ref.grad_value_l1 * (1 + 1e-12)).all())
        if name == 'edge':
            assert bool((ref.grad_mat[..., G.unreferenced, :] == 0).all())
            assert bool((ref.grad_mat_l1[..., G.unreferenced, :] == 0).all())
            assert bool((ref.out[..., :3, :] == 0).all())


@pytest.mark.parametrize('reduce', ['sum', 'mean'])
def test_grad_value_against_c_oracle(reduce):
    for name, G in _graphs():
        for batch, K in (((), 7), ((2, ), 4)):
            x = synth.features(G.N, K, seed=21, dtype=torch.float64, batch=batch)
            g = synth.features(G.M, K, seed=22, dtype=torch.float64, batch=batch)
            gv, l1 = R.grad_value(G.row, G.col, x, g, reduce, G.M)
            want = oc.spmm_value_bw(oc.F64, reduce, G.row.numpy(), G.rowptr.numpy(), G.col.numpy(), x.numpy(),
                                    g.numpy())
            assert float((gv - torch.from_numpy(want)).abs().max()) <= 1e-13 * max(1.0, float(l1.max())), name


def test_builders_keep_their_properties():
    G = R.edge_graph()  # (asserts its own list)
    deg = G.rowptr[1:] - G.rowptr[:-1]
    assert int(deg[G.hub_row]) >= 700 and int(torch.bincount(G.col, minlength=G.N)[G.hub_col]) > 512
    assert G.N == 257 and G.col.numel() % 64 != 0 and G.col.numel() % 256 != 0
    assert bool((deg[:3] == 0).all()) and bool((deg[-5:] == 0).all())
    assert bool((G.row[1:] >= G.row[:-1]).all()), 'CSR order'
    assert bool(torch.equal(torch.bincount(G.row, minlength=G.M), deg))
    tiny = R.tiny_graphs()
    assert [t.col.numel() for t in tiny] == [1, 63, 64, 65, 255, 256, 257]
    for t in tiny:
        d = t.rowptr[1:] - t.rowptr[:-1]
        assert int(d[0]) == 0 and int(d[-1]) == 0 and t.M <= 8
    colptr, perm = R.csc_arrays(G)
    assert bool((G.col[perm][1:] >= G.col[perm][:-1]).all()) and int(colptr[-1]) == G.col.numel()
    assert bool(torch.equal(torch.sort(perm).values, torch.arange(G.col.numel())))


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_width_lists_reach_every_lane_group_and_trip_count(dtype):
    """launch_value_bw restated: slots = ceil(K / VEC), lpr = min(64, next_pow2(slots)); trips = ceil(slots / lpr)."""
    es = R.element_size(dtype)

    def rule(K, vec):
        slots = -(-K // vec)
        lpr = min(64, 1 << max(0, int(slots - 1).bit_length()))
        return lpr, -(-slots // lpr)

    vec = [rule(K, 16 // es) for K in R.vector_widths(dtype)]
    sca = [rule(K, 1) for K in R.scalar_widths(dtype)]
    assert all((K * es) % 16 == 0 for K in R.vector_widths(dtype))
    assert all((K * es) % 16 != 0 for K in R.scalar_widths(dtype)) and len(R.scalar_widths(dtype)) >= 8
    assert [K // (16 // es) for K in R.vector_widths(dtype)] == list(R.VECTOR_SLOTS)
    assert {l for l, _ in vec} == {1, 2, 4, 8, 16, 32, 64}
    assert {l for l, _ in vec + sca} == {1, 2, 4, 8, 16, 32, 64}
    assert {t for _, t in vec} == {1, 2, 3} and {t for _, t in sca} == {1, 2, 3}
    # exactly one full trip, one lane into the second, a full second, one lane into the third
    slots = list(R.VECTOR_SLOTS)
    assert 64 in slots and 65 in slots and 128 in slots and 130 in slots
    for K in R.vector_widths(dtype):
        assert R.value_bw_launch(K, dtype) == rule(K, 16 // es)
        assert R.value_bw_launch(K, dtype, aligned=False) == rule(K, 1)
    for K in R.scalar_widths(dtype):
        assert R.value_bw_launch(K, dtype) == rule(K, 1)


def test_integer_inputs_are_exact_in_every_dtype():
    G = R.edge_graph()
    for dtype in FLOAT_DTYPES:
        x, g, v = R.integer_inputs(G, 130 * (16 // R.element_size(dtype)), dtype, 3, (2, ), with_value=True)
        ref = R.reference(G.row, G.col, v, x, g, 'sum', G.M)
        for t in (ref.out_l1, ref.grad_value_l1, ref.grad_mat_l1):
            assert float(t.max()) < R.FP16_MAX
        for t in (ref.out, ref.grad_value, ref.grad_mat):
            assert bool((t == t.round()).all())
    # bf16 holds integers up to 256 only: the exact results are rounded ONCE, which is what the kernels must return
    assert float(ref.grad_value.abs().max()) > 256


# ---- sensitivity ------------------------------------------------------------------------------------------------
def _sensitivity_case():
    G = R.edge_graph()
    K, batch, dtype = 20, (2, ), torch.float32
    x = synth.features(G.N, K, seed=31, dtype=dtype, batch=batch)
    g = synth.features(G.M, K, seed=32, dtype=dtype, batch=batch)
    v = R.edge_values(G.col.numel(), dtype, 33)
    return G, K, dtype, x, g, v


def test_comparator_accepts_the_plain_computation():
    G, K, dtype, x, g, v = _sensitivity_case()
    for reduce in ('sum', 'mean'):
        for value in (v, None):
            ref = R.reference(G.row, G.col, value, x, g, reduce, G.M)
            out, gv, gm = R.plain_same_precision(G.row, G.col, value, x, g, reduce, G.M)
            assert R.assert_within_bound(out, ref.out, ref.out_l1, dtype, 'out') <= 0.5
            assert R.assert_within_bound(gv, ref.grad_value, ref.grad_value_l1, dtype, 'grad_value') <= 0.5
            assert R.assert_within_bound(gm, ref.grad_mat, ref.grad_mat_l1, dtype, 'grad_mat') <= 0.5


# worst |err| / bound of the plain same-precision computation over the shapes below, as measured (the figures
# docs/design/spmm_backward.md quotes); the test recomputes them and holds them to these ceilings
PLAIN_RATIO = {torch.float32: 0.06, torch.float64: 0.02, torch.float16: 0.48, torch.bfloat16: 0.42}


@pytest.mark.parametrize('dtype', FLOAT_DTYPES)
def test_plain_computation_leaves_half_the_bound_at_the_widest_rows(dtype):
    """130 packets per row (the widest of the sweep) and the widest autograd width, batch () and (2,), sum and mean,
    with and without values: a GPU result may use up to twice what the plain computation needs, so the plain one has
    to stay under half the bound -- and under the ratio the design document states for its dtype."""
    G = R.edge_graph()
    worst = {}
    for K in (R.vector_widths(dtype)[-1], 130):
        for batch in ((), (2, )):
            x = synth.features(G.N, K, seed=2, dtype=dtype, batch=batch)
            g = synth.features(G.M, K, seed=3, dtype=dtype, batch=batch)
            v = R.edge_values(G.col.numel(), dtype)
            for reduce in ('sum', 'mean'):
                for value in (v, None):
                    ref = R.reference(G.row, G.col, value, x, g, reduce, G.M)
                    out, gv, gm = R.plain_same_precision(G.row, G.col, value, x, g, reduce, G.M)
                    for name, got, exact, l1 in (('out', out, ref.out, ref.out_l1),
                                                 ('grad_value', gv, ref.grad_value, ref.grad_value_l1),
                                                 ('grad_mat', gm, ref.grad_mat, ref.grad_mat_l1)):
                        key = '%s %s' % (reduce, name)
                        worst[key] = max(worst.get(key, 0.0), R.bound_ratio(got, exact, l1, dtype))
    print(dtype, {k: round(r, 3) for k, r in sorted(worst.items())})
    assert max(worst.values()) <= PLAIN_RATIO[dtype] <= 0.5, worst
    if dtype in (torch.float16, torch.bfloat16):
        assert max(worst, key=worst.get) == 'mean grad_mat', worst


def test_comparator_rejects_six_planted_defects():
    """Each damage is applied to the fp64 reference itself (no rounding noise at all): the bound check must still
    see it.  Nothing here is ever built for or run on a GPU."""
    G, K, dtype, x, g, v = _sensitivity_case()
    row, col, M, N = G.row, G.col, G.M, G.N
    xd, gd, vd = x.double(), g.double(), v.double()
    s = R.reference(row, col, v, x, g, 'sum', M)
    m = R.reference(row, col, v, x, g, 'mean', M)
    deg = torch.bincount(row, minlength=M)

    def rejected(got, exact, l1):
        r = R.bound_ratio(got, exact, l1, dtype)
        with pytest.raises(AssertionError):
            R.assert_within_bound(got, exact, l1, dtype)
        return r > 1.0

    assert R.bound_ratio(s.grad_value, s.grad_value, s.grad_value_l1, dtype) == 0.0
    # 1. the last 16-byte packet (four fp32 features) of a row left out of the dot product
    short, _ = R.grad_value(row, col, x[..., :K - 4], g[..., :K - 4], 'sum', M)
    assert rejected(short, s.grad_value, s.grad_value_l1)
    # 2. the last edge of the tail wave left at 0
    tail = s.grad_value.clone()
    tail[-1] = 0.0
    assert col.numel() % 64 != 0 and rejected(tail, s.grad_value, s.grad_value_l1)
    # 3. deg instead of max(deg, 1): the rows of g are scaled by 1 / deg first, the slot of an empty row holds
    #    g / 0, and the first row after an empty one also adds 0 * (its empty neighbour's slot) -- a NaN
    with np.errstate(all='ignore'):
        scaled = gd / deg.double().view(-1, 1)
    first = torch.nonzero((deg[1:] > 0) & (deg[:-1] == 0)).flatten() + 1
    assert first.numel() >= 3
    bad = m.grad_mat.clone()
    for r in first.tolist():
        for e in range(int(G.rowptr[r]), int(G.rowptr[r + 1])):
            bad[..., int(col[e]), :] += 0.0 * scaled[..., r - 1, :]
    assert rejected(bad, m.grad_mat, m.grad_mat_l1)
    # 4. one entry of the hub column dropped from grad_mat
    e = int(torch.nonzero(col == G.hub_col).flatten()[100])
    drop = s.grad_mat.clone()
    drop[..., G.hub_col, :] -= vd[e] * gd[..., int(row[e]), :]
    assert rejected(drop, s.grad_mat, s.grad_mat_l1)
    # 5. batch 1 reads batch 0's g
    g0 = g.clone()
    g0[1] = g0[0]
    wrong = R.reference(row, col, v, x, g0, 'sum', M)
    assert rejected(wrong.grad_value, s.grad_value, s.grad_value_l1)
    assert rejected(wrong.grad_mat, s.grad_mat, s.grad_mat_l1)
    # 6. the mean weight from the column's count instead of the row's
    colcnt = torch.bincount(col, minlength=N).clamp(min=1).double()
    w = vd / colcnt[col]
    byc = torch.zeros(2, N, K, dtype=torch.float64).index_add_(1, col, w.view(1, -1, 1) * gd[:, row, :])
    assert rejected(byc, m.grad_mat, m.grad_mat_l1)


def test_bound_is_the_projects_own():
    """The comparator uses tests/util.py's constants, elementwise, with the absolute floor."""
    for dtype in FLOAT_DTYPES:
        exact = torch.tensor([1.0, 0.0, -2.0], dtype=torch.float64)
        l1 = torch.tensor([3.0, 0.0, 2.0], dtype=torch.float64)
        edge = exact + torch.tensor([3.0, 0.0, 2.0]) * SUM_TOL[dtype] * 0.999
        assert R.bound_ratio(edge, exact, l1, dtype) <= 1.0
        over = exact.clone()
        over[2] += 2.0 * SUM_TOL[dtype] * 1.01 + 2 * SUM_ATOL[dtype]
        assert R.bound_ratio(over, exact, l1, dtype) > 1.0
        nz = exact.clone()
        nz[1] = 1e-3  # something where nothing is summed
        assert R.bound_ratio(nz, exact, l1, dtype) > 1.0
        assert R.bound_ratio(torch.full((3, ), float('nan'), dtype=torch.float64), exact, l1, dtype) == float('inf')
        assert R.bound_ratio(exact[:2], exact, l1, dtype) == float('inf')
