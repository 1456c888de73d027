"""tests/index_reference.py on the CPU: every oracle against a per-element Python loop on a few hundred seeded tiny
inputs, the censuses against loops that walk the kernels' index arithmetic one workgroup at a time, and every case of
tests/test_index_kernels_gpu.py against the census it is named for -- a case that no longer reaches its target fails
here, before any GPU is involved.  The sizes come from tsamd_index_route (pinned in tests/test_index_route.py)."""
import ctypes

import numpy as np
import pytest

from pytorch_sparse_amd import _native as nat
from tests import index_reference as R


def sizes():
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().tsamd_index_route(out) == 0
    return R.sizes_from_route(list(out))


SZ = sizes()
SEEDS = range(60)


def tiny_csr(rng, max_rows=7, max_len=4, empty=0.4):
    M = int(rng.integers(0, max_rows + 1))
    lens = np.where(rng.random(M) < empty, 0, rng.integers(0, max_len + 1, M))
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return M, ptr, rng.integers(0, 9, int(ptr[-1])).astype(np.int64)


# ---- oracles against loops ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', SEEDS)
def test_scan_ind2ptr_ptr2ind_against_loops(seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-5, 1 << 41, int(rng.integers(0, 12))).astype(np.int64)
    out, total = R.exclusive_scan(x)
    run = 0
    for i, v in enumerate(x.tolist()):
        assert out[i] == run
        run += v
    assert total == run and out.dtype == np.int64
    M, ptr, _ = tiny_csr(rng)
    ind = []
    for r in range(M):
        ind += [r] * int(ptr[r + 1] - ptr[r])
    assert R.ptr2ind(ptr).tolist() == ind
    assert R.ind2ptr(ind, M).tolist() == [sum(1 for v in ind if v < i) for i in range(M + 1)]
    assert R.ind2ptr(ind, M).tolist() == ptr.tolist()


@pytest.mark.parametrize('seed', SEEDS)
def test_select_against_loops(seed):
    rng = np.random.default_rng(100 + seed)
    S, ptr, ind = tiny_csr(rng)
    idx = rng.integers(-S - 2, S + 2, int(rng.integers(0, 9))).astype(np.int64)
    out_ptr, seg, got, pos, errors = [0], [], [], [], 0
    for i, j in enumerate(idx.tolist()):
        if j < 0:
            j += S
        if j < 0 or j >= S:
            errors += 1
            out_ptr.append(out_ptr[-1])
            continue
        for e in range(int(ptr[j]), int(ptr[j + 1])):
            seg.append(i)
            got.append(int(ind[e]))
            pos.append(e)
        out_ptr.append(len(seg))
    p, total, err = R.select_plan(ptr, S, idx)
    assert (p.tolist(), total, err) == (out_ptr, len(seg), errors)
    s, g, q = R.select_fill(ptr, S, ind, idx)
    assert (s.tolist(), g.tolist(), q.tolist()) == (seg, got, pos)
    assert s.dtype == g.dtype == q.dtype == np.int64


@pytest.mark.parametrize('seed', SEEDS)
def test_filter_against_loops(seed):
    rng = np.random.default_rng(200 + seed)
    n, M, N = int(rng.integers(0, 14)), 5, 6
    row = np.sort(rng.integers(0, M, n)).astype(np.int64)
    col = rng.integers(0, N, n).astype(np.int64)
    a, b = int(rng.integers(-3, 5)), int(rng.integers(0, 5))
    row_map, col_map = rng.integers(0, 50, M).astype(np.int64), rng.integers(-1, 50, N).astype(np.int64)
    for pred in R.PREDS:
        size = {'mask': n, 'mask_row': M, 'mask_col': N}.get(pred, 0)
        mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size)
        want = []
        for i in range(n):
            r, c = int(row[i]), int(col[i])
            want.append({'col_range': lambda: a <= c < a + b, 'off_diag': lambda: r != c - a, 'mask': lambda: mask[i] != 0,
                         'mask_row': lambda: mask[r] != 0, 'mask_col': lambda: mask[c] != 0,
                         'col_mapped': lambda: col_map[c] >= 0}[pred]())
        keep = R.keep_flags(pred, row, col, mask, col_map, a, b)
        assert keep.tolist() == [bool(w) for w in want]
        pos, count = R.filter_positions(keep)
        assert pos.tolist() == [sum(want[:i]) for i in range(n + 1)] and count == sum(want)
        for rm, cm, rs, cs in ((None, None, 0, 0), (row_map, col_map, 3, -2), (None, col_map, 0, 7)):
            ro, co, so = R.filter_compact(keep, row, col, rm, cm, rs, cs)
            loop = [((int(rm[row[i]]) if rm is not None else int(row[i])) - rs,
                     (int(cm[col[i]]) if cm is not None else int(col[i])) - cs, i) for i in range(n) if want[i]]
            assert list(zip(ro.tolist(), co.tolist(), so.tolist())) == loop


@pytest.mark.parametrize('seed', SEEDS)
def test_filter_inputs_realise_the_pattern(seed):
    rng = np.random.default_rng(300 + seed)
    keep = rng.random(int(rng.integers(0, 40))) < rng.random()
    for pred in R.PREDS:
        for variant in range(6):
            inp = R.filter_inputs(pred, keep, variant, seed)
            assert np.array_equal(R.keep_flags(pred, inp['row'], inp['col'], inp['mask'], inp['map'], inp['a'], inp['b']), keep)
            assert (np.diff(inp['row']) >= 0).all() and (inp['row'] >= 0).all() and (inp['row'] < inp['M']).all()
            if pred != 'off_diag':  # (its columns are only compared, never used as an index)
                assert (inp['col'] >= 0).all() and (inp['col'] < inp['N']).all()


def dense_walk(M, N, k, row, col, drop_on_diagonal):
    """the merged pattern by walking the dense M x N grid in row-major order"""
    where = {(int(r), int(c)): i for i, (r, c) in enumerate(zip(row, col))}
    E, j, out = len(row), 0, []
    for r in range(M):
        for c in range(N):
            if c == r + k:
                if (r, c) in where and not drop_on_diagonal:
                    out.append((r, c, where[(r, c)]))
                out.append((r, c, E + j))
                j += 1
            elif (r, c) in where:
                out.append((r, c, where[(r, c)]))
    return out, j


@pytest.mark.parametrize('case', R.diag_small_cases(), ids=lambda c: c[0])
def test_diag_against_a_walk_over_the_dense_grid(case):
    _, M, N, k, kind, row, col = case
    assert (np.diff(row * N + col) > 0).all()
    on = int((col - row == k).sum())
    assert {'whole': on == R.num_diag(M, N, k), 'none': on == 0, 'part': on == (R.num_diag(M, N, k) + 1) // 2}[kind]
    E = row.size
    walk, nd = dense_walk(M, N, k, row, col, drop_on_diagonal=True)
    assert R.num_diag(M, N, k) == nd == max(0, min(M + k, N) if k < 0 else min(M, N - k))
    pos, count, r, c, s = R.set_diag(row, col, M, N, k)
    assert list(zip(r.tolist(), c.tolist(), s.tolist())) == walk
    assert count == E - on and pos.tolist() == [int((col[:i] - row[:i] != k).sum()) for i in range(E + 1)]
    # the mask: off-diagonal entry i sits i + (diagonal places before it) into E + num_diag bytes
    walk_all, _ = dense_walk(M, N, k, row, col, drop_on_diagonal=False)
    mask = [1 if s < E and col[s] - row[s] != k else 0 for _, _, s in walk_all]
    assert R.non_diag_mask(row, col, M, N, k).tolist() == mask and len(mask) == E + nd
    if on == 0:
        r2, c2, s2 = R.insert_diag(row, col, M, N, k)
        assert list(zip(r2.tolist(), c2.tolist(), s2.tolist())) == walk


@pytest.mark.parametrize('case', R.scatter_cases(SZ), ids=lambda c: c[0])
def test_cat_plan_against_loops(case):
    _, M, ops = case
    out_ptr, deltas = R.cat_plan([r for r, _, _ in ops], M)
    want = sorted((int(r), int(c) + sum(w for _, _, w in ops[:o]), o, i)
                  for o, (row, col, _) in enumerate(ops) for i, (r, c) in enumerate(zip(row, col)))
    offs = np.cumsum([0] + [len(r) for r, _, _ in ops])
    slots = {}
    for o, (row, col, _) in enumerate(ops):
        assert (np.diff(row * 1000 + col) > 0).all()
        for i, r in enumerate(row.tolist()):
            slots[i + int(deltas[o][r])] = (r, int(col[i]) + sum(w for _, _, w in ops[:o]), o, i)
    assert [slots[p] for p in range(len(want))] == want            # every slot exactly once, in (row, col) order
    r, c, s = R.cat_columns(ops, M)
    assert list(zip(r.tolist(), c.tolist(), s.tolist())) == [(a, b, int(offs[o]) + i) for a, b, o, i in want]
    assert out_ptr.tolist() == R.ind2ptr(r, M).tolist()


# ---- censuses against a walk through the kernels' index arithmetic -----------------------------------------------------
def last_le(ptr, n, e):
    """segment_of (csrc/expand.h) as a linear walk: the last i in [0, n) with ptr[i] <= e"""
    return max(i for i in range(n) if ptr[i] <= e)


@pytest.mark.parametrize('seed', range(30))
def test_censuses_against_loops(seed):
    rng = np.random.default_rng(400 + seed)
    tiny = R.Sizes(scan_tile=4, expand_tile=4, filter_tile=8, filter_slice=4, long_run=3)
    M, ptr, _ = tiny_csr(rng, max_rows=12, empty=0.7)
    E = int(ptr[-1])
    got = R.expand_census(ptr, M, E, tiny)
    for t, (lo, hi, n, route) in enumerate(got):
        e0, e1 = 4 * t, min(4 * t + 4, E)
        assert (lo, hi) == (last_le(ptr, M, e0), last_le(ptr, M, e1 - 1))
        assert n == hi - lo + 1 and route == ('staged' if n <= 4 else 'search')
    assert len(got) == -(-E // 4)
    ind = R.ptr2ind(ptr)
    c = R.ind2ptr_census(ind, M, tiny)
    assert len(c) == (E + 1 if E else 0)
    owned = []
    for t, (lo, hi, run, route) in enumerate(c):
        assert lo == (0 if t == 0 else ind[t - 1] + 1) and hi == (M if t == E else ind[t])
        assert run == hi - lo + 1 and route == ('long' if hi - lo >= 3 else 'inline')
        owned += list(range(lo, hi + 1))
    assert not E or owned == list(range(M + 1))                     # every row pointer has exactly one owner
    n = int(rng.integers(0, 90))
    levels, m = [], n
    while m > 0:
        m = -(-m // 4)
        levels.append(m)
        if m == 1:
            break
    assert R.scan_census(n, tiny) == levels
    keep = rng.random(int(rng.integers(0, 30))) < 0.5
    f = R.filter_census(keep, tiny)
    assert f['tiles'] == max(1, -(-keep.size // 8)) and f['kept'] == int(keep.sum())
    assert f['slices'] == [('none', 'mixed', 'all')[int(keep[s:s + 4].any()) + int(keep[s:s + 4].all())] for s in range(0, keep.size, 4)]


def test_scan_workspace_is_what_the_levels_use():
    """tsamd_exclusive_scan_workspace_bytes = one aligned array of tile sums per level above the last + 256: a query
    that is one level short would be smaller than this"""
    L = nat.lib()
    T = SZ.scan_tile
    for n in (0, 1, T, T + 1, 2 * T + 1, T * T, T * T + 1, T * T + T + 1, 5 * T * T):
        want = R.scan_workspace_bytes(n, SZ)
        assert L.tsamd_exclusive_scan_workspace_bytes(ctypes.c_int64(n)) == want, n
        assert L.tsamd_select_workspace_bytes(ctypes.c_int64(n - 1)) == want
        assert L.tsamd_filter_workspace_bytes(ctypes.c_int64(n - 1)) == want
    for n in (0, 1, T, T + 1, T * T, T * T + 1, T * T * T):
        tiles = -(-max(n, 1) // SZ.filter_tile)
        assert L.tsamd_filter_tiles_workspace_bytes(ctypes.c_int64(n)) == \
            R.align_up(8 * (tiles + 1), 256) + R.scan_workspace_bytes(tiles + 1, SZ)


# ---- every case of the GPU file has the census it is named for -----------------------------------------------------
@pytest.mark.parametrize('case', R.scan_cases(SZ), ids=lambda c: c[0])
def test_scan_case_census(case):
    name, n, levels = case
    census = R.scan_census(n, SZ)
    assert len(census) == levels and ('levels%d' % levels) in name
    assert census == ([] if n == 0 else [1] if levels == 1 else [-(-n // SZ.scan_tile), 1] if levels == 2 else
                      [-(-n // SZ.scan_tile), 2, 1])


def test_scan_cases_reach_all_three_levels_and_the_values_pass_2_40():
    assert sorted({c[2] for c in R.scan_cases(SZ)}) == [0, 1, 2, 3]
    for n in (1, 2, 9, 4097):
        out, total = R.exclusive_scan(R.scan_values(n, 'big', 3))
        assert total > 1 << 40 and (n == 1 or out[1] > 1 << 32)
    assert R.scan_values(9, 'first').tolist() == [(1 << 40) + 3] + [0] * 8
    assert R.scan_values(9, 'last').tolist() == [0] * 8 + [(1 << 40) + 3]


@pytest.mark.parametrize('case', R.ind2ptr_cases(SZ), ids=lambda c: c[0])
def test_ind2ptr_case_census(case):
    name, M, ind, want = case
    assert (np.diff(ind) >= 0).all() and (ind >= 0).all() and (ind < M).all()
    assert R.ind2ptr_target_ok(R.ind2ptr_census(ind, M, SZ), M, want)
    assert name.endswith('-long') == bool(want['long'])


def test_ind2ptr_cases_cover_the_threshold():
    cases = R.ind2ptr_cases(SZ)
    Rn = SZ.long_run
    for where in ('front', 'middle', 'end'):
        for odd in (False, True):
            runs = {n.split('-')[1]: w for n, M, _, w in cases if n.startswith(where + '-run') and w['odd'] == odd}
            assert {k: bool(w['long']) for k, w in runs.items()} == {
                'run%d' % (Rn - 2): False, 'run%d' % (Rn - 1): False, 'run%d' % Rn: False, 'run%d' % (Rn + 1): True}
    assert {M for _, M, _, _ in cases} >= {1, 2, Rn - 1, Rn, Rn + 1, 4 * Rn, 4 * Rn + 1}
    sizes = {ind.size for _, _, ind, _ in cases}
    assert sizes >= {1, 255, 256, 257, SZ.expand_tile - 1, SZ.expand_tile, SZ.expand_tile + 1}


@pytest.mark.parametrize('case', R.ptr2ind_cases(SZ), ids=lambda c: c[0])
def test_ptr2ind_case_census(case):
    name, ptr, want = case
    M, E = ptr.size - 1, int(ptr[-1])
    census = R.expand_census(ptr, M, E, SZ)
    assert R.expand_target_ok(census, want), census
    routes = {r for _, _, _, r in census}
    assert ('search' in routes) == name.endswith('-search') and ('search' in routes or name.endswith('-staged'))


def test_ptr2ind_cases_hold_the_pair():
    T = SZ.expand_tile
    by = {n: R.expand_census(p, p.size - 1, int(p[-1]), SZ) for n, p, _ in R.ptr2ind_cases(SZ)}
    assert by['tile-over-%d-rows-staged' % T][0][2:] == (T, 'staged')
    assert by['tile-over-%d-rows-search' % (T + 1)][0][2:] == (T + 1, 'search')
    assert [r for _, _, _, r in by['hub-over-three-tiles-staged']] == ['staged'] * 3


@pytest.mark.parametrize('case', R.select_cases(SZ), ids=lambda c: c[0])
def test_select_case_census(case):
    name, idx, want = case
    ptr, S, ind, _ = R.select_source(SZ)
    plan = R.select_plan(ptr, S, idx)
    census = R.expand_census(plan[0], idx.size, plan[1], SZ)
    assert R.select_target_ok(census, plan, want), (census, plan[1:])
    routes = {r for _, _, _, r in census}
    assert ('search' in routes) == name.endswith('-search')
    assert not name.endswith('-staged') or routes == {'staged'}


def test_select_cases_cover_the_list():
    T = SZ.expand_tile
    cases = R.select_cases(SZ)
    ptr, S, _, _ = R.select_source(SZ)
    assert {w['total'] for _, _, w in cases} >= {0, 1, T - 1, T, T + 1, 2 * T + 1}
    assert {i.size for _, i, _ in cases} >= {0, 1, 256, 257}
    ids = np.concatenate([i for _, i, _ in cases])
    assert {-S - 1, -S, -1, 0, S - 1, S} <= set(ids.tolist())
    assert ptr[1] > ptr[0] and ptr[S] > ptr[S - 1]
    by = {n: w for n, _, w in cases}
    assert by['tile-over-%d-picks-staged' % T]['tiles'][0] == (T, 'staged')
    assert by['tile-over-%d-picks-search' % (T + 1)]['tiles'][0] == (T + 1, 'search')


@pytest.mark.parametrize('pattern', R.FILTER_PATTERNS)
def test_filter_case_census(pattern):
    ns = set()
    for name, n, pat, variant in R.filter_cases(SZ):
        if pat != pattern:
            continue
        ns.add(n)
        keep = R.keep_pattern(pat, n, SZ)
        assert R.filter_target_ok(pat, n, R.filter_census(keep, SZ), SZ), name
    T, s = SZ.filter_tile, SZ.filter_slice
    assert ns == {0, 1, 63, 64, 65, s - 1, s, s + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 300}


def test_filter_cases_reach_every_parameter():
    """b = 0 and a at both ends of the columns, k < 0 / 0 / > 0, the three mask bytes, -1 / 0 / a large rank"""
    seen = {p: set() for p in R.PREDS}
    for name, n, pat, variant in R.filter_cases(SZ):
        keep = R.keep_pattern(pat, n, SZ)
        for pred in R.PREDS:
            if n > 300 and pred not in ('col_range', 'mask'):
                continue
            inp = R.filter_inputs(pred, keep, variant)
            if pred == 'col_range':
                seen[pred].add((inp['a'], inp['b']))
            elif pred == 'off_diag':
                seen[pred].add(inp['a'])
            elif pred == 'col_mapped':
                seen[pred] |= {int(inp['map'].min()), int(inp['map'][inp['map'] >= 0].min()), int(inp['map'].max() > 1 << 40)}
            elif n and keep.any():
                seen[pred].add(int(inp['mask'].max()))
    assert seen['col_range'] >= {(0, 0), (50, 0), (100, 0), (0, 40), (60, 40), (30, 40)}
    assert seen['off_diag'] == {-3, 0, 5}
    assert seen['mask'] == seen['mask_row'] == seen['mask_col'] == {1, 2, 255}
    assert seen['col_mapped'] == {-1, 0, 1}


@pytest.mark.parametrize('case', R.diag_large_cases(), ids=lambda c: c[0])
def test_diag_large_case_census(case):
    _, M, N, k, kind, row, col = case
    census = R.diag_census(row.size, M, N, k)
    assert 2000 < row.size < 6000 and census['move'] > 1
    assert census['fill'] == {0: 3, 1: 3, -1: 3, 200: 3, -699: 1, 899: 1}[k]
    on = int((col - row == k).sum())
    assert on == ((R.num_diag(M, N, k) + 1) // 2 if kind == 'part' else 0)


def test_diag_small_cases_cover_the_list():
    cases = R.diag_small_cases()
    for M, N in ((3, 6), (4, 4), (6, 2)):
        ks = {k for _, m, n, k, _, _, _ in cases if (m, n) == (M, N)}
        assert ks == set(range(-(M + 1), N + 2))
    assert any(r.size == 0 for *_, r, _ in cases)
    assert {kind for _, _, _, _, kind, _, _ in cases} == {'whole', 'part', 'none'}
    # move + fill both launched in some case of every kind, and each alone
    seen = {(R.diag_census(r.size, M, N, k)['move'] > 0, R.diag_census(r.size, M, N, k)['fill'] > 0)
            for _, M, N, k, _, r, _ in cases}
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
