"""torch_sparse::hgt_sample on the GPU (the reference's csrc/cpu/hgt_sample_cpu.cpp; CPU-only there) against the NumPy
restatement tests/hgt_reference.py:

  * bit-exact parity wherever nothing is random (columns of at most 50 entries, hops that take the whole budget);
  * the budget arithmetic of the kernels through the C-ABI, exactly (fixed point, units of 2^-32);
  * the selection law: inclusion frequencies against the exact enumeration, and budget SQUARED;
  * hub graphs: the properties every output must have, reproducibility under torch.manual_seed;
  * errors without a device fault, the number of host read-backs, and the tensors HGTLoader builds from the outputs.
"""
import ctypes

import numpy as np
import pytest
import torch

import pytorch_sparse_amd  # noqa: F401  (registers the torch_sparse:: ops)
from tests.hgt_reference import (LAW_BUDGETS, LAW_K, LAW_R, MAX_NEIGHBORS, hgt_assemble, hgt_budget, hgt_expand_det,
                                 inclusion_probabilities, law_bound, split)
from tests.util import _count_syncs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
hgt = torch.ops.torch_sparse.hgt_sample
TYPES = ['a', 'b', 'c']
# 'c' is only ever a source; 'a__x__a' is a self-relation; 'c__e__b' is empty in every graph
RELS = ['a__x__a', 'b__w__a', 'a__r__b', 'c__h__a', 'c__e__b']
BIG = 10**6  # more samples than any budget holds: a hop takes the whole budget


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def todev(d):
    return {k: dev(v) for k, v in d.items()}


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def random_graph(seed, sizes, max_deg, hub=None, empty=('c__e__b', )):
    """One CSC per relation with in-degrees in [0, max_deg]: isolated nodes, duplicate entries, unsorted columns.  hub =
    (fraction, lo, hi): that fraction of the columns gets lo..hi entries (heavy columns, R-MAT-like)."""
    rng = np.random.default_rng(seed)
    colptr, row = {}, {}
    for rel in RELS:
        s, d = split(rel)
        deg = rng.integers(0, max_deg + 1, sizes[d])
        deg[rng.random(sizes[d]) < 0.2] = 0
        if hub is not None:
            pick = rng.random(sizes[d]) < hub[0]
            deg[pick] = np.minimum(hub[2], (hub[1] * (1.0 / (1.0 - rng.random(int(pick.sum())) * 0.99))).astype(np.int64))
        if rel in empty:
            deg[:] = 0
        cp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        rw = rng.integers(0, sizes[s], int(cp[-1])).astype(np.int64)
        for w in np.nonzero(deg >= 2)[0][::3]:
            rw[cp[w + 1] - 1] = rw[cp[w]]  # duplicate entry
        colptr[rel], row[rel] = cp, rw
    return colptr, row


def check_dicts(node, r, c, e, rels):
    for d in (r, c, e):
        assert sorted(d) == sorted(rels)
    for t in list(node.values()) + list(r.values()) + list(c.values()) + list(e.values()):
        assert t.dtype == torch.long and t.is_cuda and t.dim() == 1


def assert_edges_equal(got, want, rels):
    for rel in rels:
        for name, g, w in zip(('row', 'col', 'edge'), got[rel], want[rel]):
            assert np.array_equal(g, w), (rel, name, g[:20], w[:20])


# ---- deterministic parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2, 3, 4, 5])
def test_whole_budget_hops_against_the_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    sizes = {'a': int(rng.integers(100, 600)), 'b': int(rng.integers(40, 300)), 'c': int(rng.integers(5, 60))}
    no_c = seed % 3 == 2  # nothing reaches type 'c': it must be absent from node_dict
    colptr, row = random_graph(seed, sizes, [4, 9, MAX_NEIGHBORS][seed % 3], empty=('c__e__b', 'c__h__a') if no_c else ('c__e__b', ))
    num_hops = 1 + (seed // 2) % 3
    ia = rng.integers(0, sizes['a'], 6)
    inputs = {'a': np.concatenate([ia, ia[:2], ia[:1]])}  # ids listed twice and three times
    if seed % 2:
        inputs['b'] = rng.integers(0, sizes['b'], 3)
    node, r, c, e = hgt(todev(colptr), todev(row), todev(inputs), {t: [BIG] * num_hops for t in TYPES}, num_hops)
    check_dicts(node, r, c, e, RELS)
    node, r, c, e = host(node), host(r), host(c), host(e)
    blocks = hgt_expand_det(colptr, row, inputs, TYPES, num_hops)
    for t in TYPES:
        want_len = sum(len(b) for b in blocks[t])
        if want_len == 0:
            assert t not in node
            continue
        got = node[t]
        assert len(got) == want_len, (t, len(got), want_len)
        n_in = len(blocks[t][0])
        assert got[:n_in].tolist() == blocks[t][0]  # the inputs, in the given order, duplicates kept
        pos = n_in
        for b in blocks[t][1:]:
            part = got[pos:pos + len(b)].tolist()
            assert len(set(part)) == len(part) and set(part) == b, (t, pos)
            pos += len(b)
    if no_c:
        assert 'c' not in node
    lists = {t: node.get(t, np.zeros(0, np.int64)) for t in TYPES}
    want = hgt_assemble(colptr, row, lists)
    assert_edges_equal({rel: (r[rel], c[rel], e[rel]) for rel in RELS}, want, RELS)
    assert sum(len(r[rel]) for rel in RELS) > 0


# ---- the kernels' budget arithmetic through the C-ABI -------------------------------------------------------------------
def test_budget_words_through_the_cabi():
    from pytorch_sparse_amd import _native as nat
    L = nat.lib()
    L.tsamd_sample_workspace_bytes.restype = ctypes.c_size_t
    rng = np.random.default_rng(5)
    Ms, Md = 700, 400
    deg = rng.integers(0, MAX_NEIGHBORS + 1, Md)
    deg[::5] = 0
    cp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    rw = rng.integers(0, Ms, int(cp[-1])).astype(np.int64)
    seen = rng.permutation(Ms)[:150].astype(np.int64)
    frontier = np.concatenate([rng.permutation(Md)[:120], [3, 3, 8]]).astype(np.int64)  # a column may be expanded twice
    want = hgt_budget({'s__r__d': cp}, {'s__r__d': rw}, {'s': seen, 'd': frontier})['s']
    assert len(want) > 100

    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    I = lambda x: ctypes.c_int64(int(x))  # noqa: E731
    st = nat.stream_ptr(torch.device(DEV, 0))
    F = len(frontier)
    d_cp, d_rw, d_seen, d_fr = dev(cp), dev(rw), dev(seen), dev(frontier)
    word = torch.zeros(Ms, dtype=torch.long, device=DEV)
    cand = torch.full((Ms, ), -1, dtype=torch.long, device=DEV)
    state = torch.zeros(2, dtype=torch.long, device=DEV)
    out_ptr = torch.empty(F + 1, dtype=torch.long, device=DEV)
    info = torch.empty(2, dtype=torch.long, device=DEV)
    ws = torch.empty(max(256, L.tsamd_sample_workspace_bytes(I(F))), dtype=torch.uint8, device=DEV)
    nbr = torch.empty(F * MAX_NEIGHBORS, dtype=torch.long, device=DEV)
    e_id = torch.empty(F * MAX_NEIGHBORS, dtype=torch.long, device=DEV)
    nat.check(L.tsamd_hgt_seen(P(d_seen), I(len(seen)), I(Ms), P(word), P(state[1:]), st), 'seen')
    nat.check(L.tsamd_sample_plan(P(d_cp), I(Md), P(d_fr), I(F), I(MAX_NEIGHBORS), ctypes.c_int(0), P(out_ptr), P(info), P(ws),
                                  ctypes.c_size_t(ws.numel()), st), 'plan')
    nat.check(L.tsamd_sample_draw(P(d_cp), P(d_rw), P(d_fr), I(F), I(MAX_NEIGHBORS), ctypes.c_int(0), ctypes.c_uint64(1),
                                  P(out_ptr), P(e_id), P(nbr), st), 'draw')
    nat.check(L.tsamd_hgt_budget_add(P(out_ptr), I(F), P(nbr), I(Ms), P(word), P(cand), I(Ms), P(state), st), 'budget_add')
    word, cand, state = word.cpu().numpy(), cand.cpu().numpy(), state.cpu().numpy()
    assert state[1] == 0 and state[0] == len(want)
    exp = np.zeros(Ms, np.int64)
    for v, b in want.items():
        exp[v] = b
    exp[seen] = -1  # all-ones: seen
    assert np.array_equal(word, exp)
    assert sorted(cand[:state[0]].tolist()) == sorted(want)


def test_select_does_not_depend_on_the_order_of_the_candidate_list():
    """tsamd_hgt_select through the C-ABI: the candidate list is appended to in arbitrary order, so the winners and their
    order must be a function of (seed, hop, type tag) and the words alone; dead entries (seen) never win."""
    from pytorch_sparse_amd import _native as nat
    L = nat.lib()
    L.tsamd_hgt_select_workspace_bytes.restype = ctypes.c_size_t
    g = torch.Generator().manual_seed(3)
    M, C, k = 5000, 1200, 100
    cand = torch.randperm(M, generator=g)[:C]
    budget = torch.randint(1, 1 << 36, (C, ), generator=g)
    dead = cand[::7]
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    I = lambda x: ctypes.c_int64(int(x))  # noqa: E731
    st = nat.stream_ptr(torch.device(DEV, 0))
    outs = []
    for order in (torch.arange(C), torch.randperm(C, generator=g), torch.arange(C).flip(0)):
        word = torch.zeros(M, dtype=torch.long)
        word[cand] = budget
        word[dead] = -1
        word, d_cand = word.to(DEV), cand[order].contiguous().to(DEV)
        out = torch.empty(k, dtype=torch.long, device=DEV)
        err = torch.zeros(1, dtype=torch.long, device=DEV)
        ws = torch.empty(L.tsamd_hgt_select_workspace_bytes(I(C)), dtype=torch.uint8, device=DEV)
        nat.check(L.tsamd_hgt_select(P(d_cand), I(C), P(word), I(M), I(k), ctypes.c_uint64(99), I(1), I(2), P(out), P(err), P(ws),
                                     ctypes.c_size_t(ws.numel()), st), 'select')
        assert int(err.item()) == 0
        outs.append(out.cpu())
        assert (word.cpu()[outs[-1]] == -1).all()  # the winners turned seen
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert len(set(outs[0].tolist())) == k and not set(outs[0].tolist()) & set(dead.tolist())
    assert set(outs[0].tolist()) <= set(cand.tolist())


# ---- the selection law ---------------------------------------------------------------------------------------------------
def budget_graph(terms):
    """One type 'a', relation a__r__a: candidate i gets the budget sum(m / d for (d, m) in terms[i]) from input nodes
    whose columns hold the candidate m times and the input node itself (seen: no budget) d - m times."""
    P = len(terms)
    cols = [[] for _ in range(P)]  # the candidates have no in-edges
    inputs = []
    for i, ts in enumerate(terms):
        for (d, m) in ts:
            w = P + len(inputs)
            inputs.append(w)
            cols.append([i] * m + [w] * (d - m))
    cp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rw = np.array([v for c in cols for v in c], np.int64)
    return {'a__r__a': cp}, {'a__r__a': rw}, np.array(inputs, np.int64)


def selection_counts(terms, k, R):
    colptr, row, inputs = budget_graph(terms)
    C, Rw, In = todev(colptr), todev(row), {'a': dev(inputs)}
    drawn = []
    for i in range(R):
        torch.manual_seed(i)
        node = hgt(C, Rw, In, {'a': [k]}, 1)[0]['a']
        assert node.numel() == len(inputs) + k
        drawn.append(node[len(inputs):])
    drawn = torch.stack(drawn).cpu().numpy()
    assert (np.sort(drawn, axis=1)[:, 1:] != np.sort(drawn, axis=1)[:, :-1]).all()  # without replacement
    return np.bincount(drawn.ravel(), minlength=len(terms))[:len(terms)].astype(np.float64), drawn


def test_selection_follows_the_sequential_law():
    """Inclusion counts of R calls against the exact enumeration: |count - R pi| <= 5 sqrt(R pi (1 - pi)) + 1 for every
    candidate (tests/test_hgt_sample_ops.py holds torch.multinomial to the same bound on the same vector)."""
    terms = [[(2, 1)], [(3, 1)], [(4, 1)], [(5, 1)], [(2, 1), (3, 1)], [(3, 1), (4, 1)], [(5, 2)], [(4, 1), (5, 1)],
             [(6, 1)], [(3, 1), (50, 1)]]
    assert np.allclose([sum(m / d for d, m in ts) for ts in terms], LAW_BUDGETS)
    fixed = np.array([sum(m * ((1 << 32) // d) for d, m in ts) for ts in terms], np.float64) / 2.0**32
    pi = inclusion_probabilities(np.square(fixed), LAW_K)
    assert (LAW_R * pi >= 50).all() and (LAW_R * (1 - pi) >= 50).all()
    count, drawn = selection_counts(terms, LAW_K, LAW_R)
    ratio = np.abs(count - LAW_R * pi) / law_bound(LAW_R, pi)
    print('counts', count.tolist(), 'expected', np.round(LAW_R * pi, 1).tolist(), 'largest deviation / bound %.3f' % ratio.max())
    assert (ratio <= 1.0).all(), (count, LAW_R * pi)
    # the FIRST draw alone is proportional to budget^2
    p1 = np.square(fixed) / np.square(fixed).sum()
    first = np.bincount(drawn[:, 0], minlength=len(terms)).astype(np.float64)
    ok = (LAW_R * p1 >= 50)
    r1 = np.abs(first - LAW_R * p1) / law_bound(LAW_R, p1)
    print('first draws', first.tolist(), 'expected', np.round(LAW_R * p1, 1).tolist(), 'largest %.3f' % r1[ok].max())
    assert (r1[ok] <= 1.0).all()


def test_selection_weight_is_the_budget_squared():
    """Two candidates of budgets b and 2b, one draw: 1 : 4 (the square), not 1 : 2."""
    R = LAW_R
    count, _ = selection_counts([[(4, 1)], [(2, 1)]], 1, R)
    print('counts', count.tolist())
    assert abs(count[1] - 0.8 * R) <= law_bound(R, 0.8), count
    assert abs(count[1] - 2.0 / 3.0 * R) > law_bound(R, 2.0 / 3.0)


# ---- hub graphs ----------------------------------------------------------------------------------------------------------
HUB_SIZES = {'a': 20000, 'b': 8000, 'c': 600}


def hub_case():
    colptr, row = random_graph(77, HUB_SIZES, 12, hub=(0.05, 51, 5000))
    assert max(int(np.diff(cp).max()) for cp in colptr.values()) > 1000
    rng = np.random.default_rng(3)
    heavy = np.nonzero(np.diff(colptr['a__x__a']) > MAX_NEIGHBORS)[0][:8]
    ia = np.concatenate([rng.permutation(HUB_SIZES['a'])[:56], heavy])
    inputs = {'a': np.concatenate([ia, ia[:3]]), 'b': rng.permutation(HUB_SIZES['b'])[:16]}
    num_samples = {'a': [40, 50, 60], 'b': [30, 30, 30], 'c': [10, 10, 10]}
    return colptr, row, inputs, num_samples, 3


def test_hub_graph_properties():
    colptr, row, inputs, num_samples, num_hops = hub_case()
    torch.manual_seed(11)
    node, r, c, e = hgt(todev(colptr), todev(row), todev(inputs), num_samples, num_hops)
    check_dicts(node, r, c, e, RELS)
    node, r, c, e = host(node), host(r), host(c), host(e)
    n_in = {t: len(inputs.get(t, ())) for t in TYPES}
    for t in TYPES:
        got = node[t]
        assert got[:n_in[t]].tolist() == list(inputs.get(t, ()))
        new = got[n_in[t]:]
        assert len(new) <= sum(num_samples[t])  # every block holds at most num_samples[t][hop] nodes
        assert len(set(new.tolist())) == len(new) and not set(new.tolist()) & set(got[:n_in[t]].tolist())
    # the budgets of 'a' and 'b' are far larger than the samples: every block is full, so its bounds are known
    for t in ('a', 'b'):
        assert len(node[t]) == n_in[t] + sum(num_samples[t])
    full = {t: len(node[t]) == n_in[t] + sum(num_samples[t]) for t in TYPES}

    def listed_before(t, hop):  # what was listed when hop `hop` drew (all of it when the blocks' bounds are unknown)
        return node[t][:n_in[t] + sum(num_samples[t][:hop])] if full[t] else node[t]

    for t in TYPES:
        for hop in range(num_hops):
            if not full[t] and hop > 0:
                continue
            lo = n_in[t] + sum(num_samples[t][:hop])
            block = node[t][lo:lo + num_samples[t][hop]] if full[t] else node[t][n_in[t]:]
            reach = set()
            for rel in RELS:
                s, d = split(rel)
                if s != t:
                    continue
                before = listed_before(d, hop) if full[t] else node[d]
                for w in before:
                    reach.update(row[rel][colptr[rel][w]:colptr[rel][w + 1]].tolist())
            assert set(block.tolist()) <= reach, (t, hop)
    small = hgt_assemble(colptr, row, node, only_small=True)
    n_big = 0
    for rel in RELS:
        s, d = split(rel)
        cp, rw = colptr[rel], row[rel]
        rr, cc, ee = r[rel], c[rel], e[rel]
        assert len(rr) == len(cc) == len(ee)
        assert (np.diff(cc) >= 0).all()
        w = node[d][cc]
        assert ((ee >= cp[w]) & (ee < cp[w + 1])).all()  # an entry of the column of the node col names
        assert np.array_equal(rw[ee], node[s][rr])  # ... whose source is the node row names
        last = {int(v): i for i, v in enumerate(node[s])}
        assert rr.tolist() == [last[int(v)] for v in rw[ee]]  # a node listed twice: its last position
        big = (cp[w + 1] - cp[w]) > MAX_NEIGHBORS
        assert_edges_equal({rel: (rr[~big], cc[~big], ee[~big])}, small, [rel])
        for i in np.unique(cc[big]):
            pos = ee[cc == i]
            assert len(pos) <= MAX_NEIGHBORS and len(set(pos.tolist())) == len(pos)
            n_big += 1
    assert n_big > 10


def test_hub_graph_is_reproducible_under_manual_seed():
    colptr, row, inputs, num_samples, num_hops = hub_case()
    C, Rw, In = todev(colptr), todev(row), todev(inputs)
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        outs.append([host(d) for d in hgt(C, Rw, In, num_samples, num_hops)])
    for d1, d2 in zip(outs[0], outs[1]):
        assert sorted(d1) == sorted(d2)
        for k in d1:
            assert np.array_equal(d1[k], d2[k]), k
    assert any(not np.array_equal(outs[0][0][t], outs[2][0][t]) for t in TYPES)


def test_degenerate_calls():
    """No hops: the inputs and the edges among them.  No inputs: nothing.  Zero samples: no node beyond the inputs."""
    sizes = {'a': 200, 'b': 80, 'c': 10}
    colptr, row = random_graph(21, sizes, 9)
    C, Rw = todev(colptr), todev(row)
    inputs = {'a': np.arange(0, 60, 2), 'b': np.array([5, 5, 7])}
    for num_hops, ns in ((0, {t: [] for t in TYPES}), (2, {t: [0, 0] for t in TYPES})):
        node, r, c, e = hgt(C, Rw, todev(inputs), ns, num_hops)
        check_dicts(node, r, c, e, RELS)
        node = host(node)
        assert sorted(node) == ['a', 'b'] and all(np.array_equal(node[t], inputs[t]) for t in node)
        want = hgt_assemble(colptr, row, node)
        assert_edges_equal({rel: (r[rel].cpu().numpy(), c[rel].cpu().numpy(), e[rel].cpu().numpy()) for rel in RELS}, want, RELS)
        assert sum(len(w[0]) for w in want.values()) > 0
    node, r, c, e = hgt(C, Rw, {}, {t: [5, 5] for t in TYPES}, 2)
    check_dicts(node, r, c, e, RELS)
    assert len(node) == 0 and all(e[rel].numel() == 0 for rel in RELS)


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_device_usable():
    sizes = {'a': 300, 'b': 100, 'c': 20}
    colptr, row = random_graph(9, sizes, 6)
    C, Rw = todev(colptr), todev(row)
    ns = {t: [20, 20] for t in TYPES}
    good = {'a': dev([1, 2, 3])}
    for bad in ([1, -4, 3], [1, sizes['a'] + 7, 3]):
        with pytest.raises(IndexError):
            hgt(C, Rw, {'a': dev(bad)}, ns, 2)
        assert hgt(C, Rw, good, ns, 2)[0]['a'].numel() >= 3
    bad_row = dict(row)
    bad_row['b__w__a'] = row['b__w__a'].copy()
    bad_row['b__w__a'][len(bad_row['b__w__a']) // 2:] = -2
    with pytest.raises(IndexError):
        hgt(C, todev(bad_row), {'a': dev(np.arange(sizes['a']))}, ns, 2)
    assert hgt(C, Rw, good, ns, 2)[0]['a'].numel() >= 3
    with pytest.raises(RuntimeError, match='unknown node type'):
        hgt(C, Rw, good, {'a': [5, 5], 'b': [5, 5]}, 2)  # relations name 'c'
    with pytest.raises(RuntimeError, match='unknown node type'):
        hgt(C, Rw, {'zzz': dev([0])}, ns, 2)
    with pytest.raises(RuntimeError, match='src__rel__dst'):
        hgt({'a__a': C['a__x__a']}, {'a__a': Rw['a__x__a']}, good, ns, 2)
    with pytest.raises(RuntimeError, match='fewer than num_hops'):
        hgt(C, Rw, good, {'a': [5, 5], 'b': [5], 'c': [5, 5]}, 2)
    assert hgt(C, Rw, good, ns, 2)[0]['a'].numel() >= 3


# ---- host read-backs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('num_hops', [2, 4])
def test_host_read_backs(num_hops):
    """3 + num_hops per call once the graph's id maxima are remembered: the set-up's input maxima, one per budget update
    (num_hops of them), two for the edges -- on five relations and on one relation alike."""
    colptr, row, inputs, _, _ = hub_case()
    ns = {t: [25] * num_hops for t in TYPES}
    counts = []
    for rels in (RELS, ['a__x__a']):
        C, Rw = todev({k: colptr[k] for k in rels}), todev({k: row[k] for k in rels})
        In = {'a': dev(inputs['a'])}
        call = lambda: hgt(C, Rw, In, ns, num_hops)  # noqa: E731
        call()  # first call: fills the cache of the graph's id maxima
        _, probe = _count_syncs(lambda: torch.ones(3, device=DEV).sum().item())
        assert probe >= 1  # the counter sees a read-back
        out, n_sync = _count_syncs(call)
        assert out[0]['a'].numel() == len(inputs['a']) + 25 * num_hops
        counts.append(n_sync)
    assert counts[0] == counts[1] and counts[0] <= 3 + num_hops, counts


# ---- what HGTLoader does with the outputs ----------------------------------------------------------------------------------
def test_loader_flow():
    colptr, row, inputs, num_samples, num_hops = hub_case()
    C, Rw = todev(colptr), todev(row)
    torch.manual_seed(2)
    node, r, c, e = hgt(C, Rw, todev(inputs), num_samples, num_hops)
    feat = {t: torch.arange(HUB_SIZES[t], device=DEV, dtype=torch.float32).view(-1, 1) * torch.tensor([[1.0, -1.0]], device=DEV)
            for t in TYPES}
    x = {t: feat[t][node[t]] for t in node}
    for rel in RELS:
        s, d = split(rel)
        edge_index = torch.stack([r[rel], c[rel]])
        assert edge_index.shape == (2, e[rel].numel())
        if e[rel].numel() == 0:
            continue
        src_id = Rw[rel][e[rel]]  # the stored edge's source v; its destination w owns the column the edge lies in
        dst_id = torch.searchsorted(C[rel], e[rel], right=True) - 1
        assert torch.equal(x[s][edge_index[0]][:, 0], src_id.float())
        assert torch.equal(x[d][edge_index[1]][:, 0], dst_id.float())
