"""The HIP partitioner against its numpy restatement (tests/partition_oracle.py), bit for bit: every phase op, every
C-ABI stage of a refinement round on explicit arrays, the round loop after 1 ... 8 rounds and the whole call.  Every
comparison is np.array_equal on int64 arrays; tests/test_partition_oracle.py checks on the CPU that each input reaches
the branch it is named for (the oracle's counters), so none of these can pass vacuously."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pytorch_sparse_amd as ts
from pytorch_sparse_amd import _native as nat
from tests import partition_cases as pc
from tests import partition_oracle as po

pytestmark = pytest.mark.gpu
OPS = torch.ops.tsamd


def t64(x, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int64))).to(dev)


def csr_dev(A, dev):
    A = po.csr(A)
    return t64(A.indptr, dev), t64(A.indices, dev), t64(A.data, dev)


def same(got, want, what=''):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == np.int64 and want.dtype == np.int64 and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert np.array_equal(got, want), '%s: %d differ, first at %s: got %s, want %s' % (
        what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


cases = functools.lru_cache(None)(lambda family: getattr(pc, family)())


# ---- the C-ABI stages of a refinement round ---------------------------------------------------------------------------
class Stages:
    """tsamd_partition_* on torch tensors; every call returns new tensors (the inputs stay as they are)."""

    def __init__(self, dev):
        self.dev, self.L = dev, nat.lib()
        for name in ('conn', 'commit'):
            getattr(self.L, 'tsamd_partition_%s_workspace_bytes' % name).restype = ctypes.c_size_t

    def empty(self, n):
        return torch.empty(n, dtype=torch.long, device=self.dev)

    def dev64(self, x):
        return None if x is None else t64(x, self.dev)

    def run(self, name, *args):
        """args: device tensors or None (pointers), Python ints (int64), ctypes values (as they are).  The tensors stay
        referenced until the call has finished on the device."""
        conv = [ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else
                ctypes.c_int64(a) if isinstance(a, int) else a for a in args]
        nat.check(getattr(self.L, 'tsamd_partition_' + name)(*conv, nat.stream_ptr(self.dev)), name)
        torch.cuda.synchronize(self.dev)

    def conn(self, A, vw, part, pw, k, cap, mode, lightest):
        rowptr, col, w = csr_dev(A, self.dev)
        n = A.shape[0]
        dest, gain = self.empty(n), self.empty(n)
        ws = nat.workspace(self.L.tsamd_partition_conn_workspace_bytes(ctypes.c_int64(n), ctypes.c_int64(k)), self.dev)
        self.run('conn', rowptr, col, w, self.dev64(vw), self.dev64(part), self.dev64(pw), n, k, int(cap), ctypes.c_int(mode),
                 None if lightest is None else self.dev64([lightest]), dest, gain, ws, ctypes.c_size_t(ws.numel()))
        return dest, gain

    def coo(self, A):
        return tuple(self.dev64(x) for x in po.coo_of(po.csr(A)))

    def recount(self, A, part, pw, gain, cap, dest):
        r, c, w = self.coo(A)
        n = A.shape[0]
        dest, acc = self.dev64(dest), self.empty(n)
        self.run('recount', r, c, w, self.dev64(part), self.dev64(pw), self.dev64(gain), n, r.numel(), int(cap), dest, acc)
        return dest, acc

    def commit(self, dest, gain, vw, part, pw, k, cap, select):
        n = len(dest)
        dest = self.dev64(dest)
        ws = nat.workspace(self.L.tsamd_partition_commit_workspace_bytes(ctypes.c_int64(n), ctypes.c_int64(k)), self.dev)
        self.run('commit', dest, self.dev64(gain), self.dev64(vw), self.dev64(part), self.dev64(pw), n, k, int(cap),
                 ctypes.c_int(select), ws, ctypes.c_size_t(ws.numel()))
        return dest

    def apply(self, dest, vw, part, pw, k):
        part, pw, moved = self.dev64(part), self.dev64(pw), self.dev64([0])
        self.run('apply', self.dev64(dest), self.dev64(vw), len(dest), k, part, pw, moved)
        return part, pw, int(moved.item())

    def cut(self, A, part):
        r, c, w = self.coo(A)
        out = self.dev64([-7])
        self.run('cut', r, c, w, self.dev64(part), r.numel(), out)
        return int(out.item())

    def balance(self, pw, cap):
        out = self.dev64([-7, -7, -7])
        self.run('balance', self.dev64(pw), len(pw), int(cap), out)
        return tuple(out.tolist())

    def keep_better(self, cuts, over, part_old, pw_old, part, pw):
        cuts, part, pw = self.dev64(cuts), self.dev64(part), self.dev64(pw)
        self.run('keep_better', cuts, self.dev64([over]), self.dev64(part_old), self.dev64(pw_old), len(part), len(pw), part, pw)
        return part, pw, cuts.tolist()


@pytest.fixture(scope='module')
def stages(dev):
    return Stages(dev)


# ---- matching -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['unit_grid', 'rmat9', 'hubs'])
def test_match_equals_the_oracle_after_every_round(dev, name):
    A, vw, cap = cases('match_cases')[name]
    rowptr, col, w = csr_dev(A, dev)
    states = list(po.match_rounds(A, vw, cap, 4))
    for rounds in (1, 2, 3, 4):
        match, cmap, n_c = OPS.partition_match(rowptr, col, w, t64(vw, dev), cap, rounds)
        want = states[rounds]
        same(match, want[0], 'match after %d rounds' % rounds)
        same(cmap, want[1], 'cmap after %d rounds' % rounds)
        assert n_c.tolist() == [want[2]]
    assert states[4][2] <= states[1][2] < A.shape[0]


# ---- initial partition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['grid_k5', 'grid_k7', 'five_components', 'k_above_n', 'no_edges', 'zero_weights', 'seed_tie'])
def test_initial_equals_the_oracle(dev, name):
    A, vw, k = cases('initial_cases')[name]
    rowptr, col, _ = csr_dev(A, dev)
    same(OPS.partition_initial(rowptr, col, t64(vw, dev), k), po.initial(A, vw, k), name)


# ---- connectivity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_conn_equals_the_oracle_on_every_route(stages, mode):
    A, vw, part, _ = cases('conn_graph')
    k = pc.CONN_K
    pw = po.part_weights(part, vw, k)
    for cap in pc.CONN_CAPS:
        lightest = po.balance(pw, cap)[2]
        # mode 2: the lightest part, then (in its place) the blocked hubs' own part and a full part: no fall-back
        for l in ([lightest, 200, int(np.argmax(pw))] if mode == 2 else [None]):
            dest, gain = stages.conn(A, vw, part, pw, k, cap, mode, l)
            want = po.conn(A, vw, part, pw, k, cap, mode, l)
            same(dest, want[0], 'dest, mode %d cap %d lightest %s' % (mode, cap, l))
            same(gain, want[1], 'gain, mode %d cap %d lightest %s' % (mode, cap, l))


# ---- recount, commit, apply, balance, cut, keep_better ---------------------------------------------------------------
def test_recount_equals_the_oracle(stages):
    for name in ('grid_k4_random', 'rmat_k7_unit', 'two_parts_over'):
        A, vw, part, k, cap = cases('refine_cases')[name]
        pw = po.part_weights(part, vw, k)
        po.reset_counters()
        for mode in (0, 1):
            dest, gain = po.conn(A, vw, part, pw, k, cap, mode)
            want = po.recount(A, part, pw, gain, cap, dest)
            assert (want[0] >= 0).sum() > 0
            got = stages.recount(A, part, pw, gain, cap, dest)
            same(got[0], want[0], 'dest ' + name)
            same(got[1], want[1], 'acc ' + name)
        assert po.COUNTERS['recount_dropped'] > 0


@pytest.mark.parametrize('select', [0, 1])
def test_commit_equals_the_oracle(stages, select):
    dest, gain, vw, part, pw, k, cap = cases('commit_inputs')
    same(stages.commit(dest, gain, vw, part, pw, k, cap, select), po.commit(dest, gain, vw, part, pw, k, cap, select))
    nothing = np.full(dest.size, -1, np.int64)
    same(stages.commit(nothing, gain, vw, part, pw, k, cap, select), nothing, 'no vertex has a destination')
    # the candidates of a real round, and those of a rebalance pass (select 1, then 0 on its result)
    A, vw, part, k, cap = cases('refine_cases')['all_in_part_0_random' if select else 'grid_k7_random']
    pw = po.part_weights(part, vw, k)
    dest, gain = po.conn(A, vw, part, pw, k, cap, 2 if select else 0, po.balance(pw, cap)[2])
    want = po.commit(dest, gain, vw, part, pw, k, cap, select)
    assert 0 < (want >= 0).sum() < (dest >= 0).sum()
    same(stages.commit(dest, gain, vw, part, pw, k, cap, select), want)
    if select:
        same(stages.commit(want, gain, vw, part, pw, k, cap, 0), po.commit(want, gain, vw, part, pw, k, cap, 0))


def test_apply_cut_balance_equal_the_oracle(stages):
    A, vw, part, k, cap = cases('refine_cases')['rmat_k7_random']
    pw = po.part_weights(part, vw, k)
    dest, gain = po.conn(A, vw, part, pw, k, cap, 0)
    dest = po.commit(dest, gain, vw, part, pw, k, cap, 0)
    dest[:5] = part[:5]  # a destination equal to the own part moves nothing
    want = po.apply(dest, vw, part, pw, k)
    got = stages.apply(dest, vw, part, pw, k)
    assert want[2] > 0 and got[2] == want[2]
    same(got[0], want[0], 'part')
    same(got[1], want[1], 'pw')
    assert stages.cut(A, part) == po.cut(A, part) > 0 and stages.cut(A, want[0]) == po.cut(A, want[0])
    assert stages.cut(A, np.zeros_like(part)) == 0
    for pws, c in ((pw, cap), (pw, int(pw.min())), (want[1], int(np.median(pw))), (np.array([9, 4, 12, 4, 11]), 10),
                   (np.arange(700, 0, -1), 350)):
        assert stages.balance(pws, c) == po.balance(pws, c)


@pytest.mark.parametrize('cuts,over', [((10, 12), 0), ((10, 12), 1), ((10, 10), 0), ((10, 8), 1), ((10, 8), 0)])
def test_keep_better_equals_the_oracle(stages, cuts, over):
    rs = np.random.RandomState(0)
    n, k = 700, 300   # more than one block of vertices and of parts
    part_old, part = rs.randint(0, k, n), rs.randint(0, k, n)
    pw_old, pw = rs.randint(0, 9, k), rs.randint(0, 9, k)
    want = po.keep_better(list(cuts), over, part_old, pw_old, part, pw)
    got = stages.keep_better(cuts, over, part_old, pw_old, part, pw)
    same(got[0], want[0], 'part')
    same(got[1], want[1], 'pw')
    assert got[2] == want[2]
    assert np.array_equal(want[0], part_old) == (cuts[1] > cuts[0] and over == 0)


# ---- the rounds of a level ------------------------------------------------------------------------------------------
def check_refine(dev, A, vw, start, k, cap, all_rounds=range(1, 9)):
    rowptr, col, w = csr_dev(A, dev)
    for rounds in all_rounds:
        out, dest, gain = OPS.partition_refine(rowptr, col, w, t64(vw, dev), t64(start, dev), k, cap, rounds)
        want = po.refine(A, vw, start, k, cap, rounds)
        same(out, want[0], 'part after %d rounds' % rounds)
        same(dest, want[1], 'dest of round 0')
        same(gain, want[2], 'gain of round 0')


@pytest.mark.parametrize('weights', ['unit', 'random'])
@pytest.mark.parametrize('k', [2, 4, 7])
@pytest.mark.parametrize('graph', ['grid', 'rmat'])
def test_refine_equals_the_oracle_after_every_round(dev, graph, k, weights):
    check_refine(dev, *cases('refine_cases')['%s_k%d_%s' % (graph, k, weights)])


@pytest.mark.parametrize('name', ['all_in_part_0_unit', 'all_in_part_0_random', 'two_parts_over'])
def test_refine_from_over_weight_starts_equals_the_oracle(dev, name):
    check_refine(dev, *cases('refine_cases')[name])


def test_an_undone_round_equals_the_oracle(dev):
    A, vw, part, k, cap = cases('undone_round')
    po.reset_counters()
    assert np.array_equal(po.refine(A, vw, part, k, cap, 1)[0], part) and po.COUNTERS['rounds_undone'] == 1
    check_refine(dev, A, vw, part, k, cap, all_rounds=(1, 2, 3, 4))


# ---- the whole call -------------------------------------------------------------------------------------------------
def opt(x, dev):
    return None if x is None else t64(x, dev)


@pytest.mark.parametrize('name', ['grid64_k2', 'grid64_k8', 'grid48x80_k5', 'ring256x8_k4', 'rmat12_k16', 'planted_weighted',
                                  'grid30x31_node_weights', 'rmat9_unsymmetric_self_loops', 'grid96_k300', 'k_above_n'])
def test_partition_equals_the_oracle(dev, name):
    rowptr, col, value, nw, k = cases('whole_cases')[name]
    got = torch.ops.torch_sparse.partition2(t64(rowptr, dev), t64(col, dev), opt(value, dev), opt(nw, dev), k, False)
    same(got, po.partition(rowptr, col, value, nw, k), name)


def test_sparse_tensor_partition_is_the_stable_sort_of_the_oracle(dev):
    rowptr, col, value, nw, k = cases('whole_cases')['grid30x31_node_weights']
    n = rowptr.size - 1
    src = ts.SparseTensor(rowptr=t64(rowptr, dev), col=t64(col, dev), sparse_sizes=(n, n), is_sorted=True)
    _, partptr, perm = src.partition(k, node_weight=torch.from_numpy(nw))
    cluster = po.partition(rowptr, col, None, nw, k)
    same(perm, np.argsort(cluster, kind='stable').astype(np.int64), 'perm')
    same(partptr, np.concatenate([[0], np.cumsum(np.bincount(cluster, minlength=k))]).astype(np.int64), 'partptr')
