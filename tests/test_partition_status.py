"""The status code of every tsamd_partition_* entry (csrc/partition.hip) for every argument it refuses -- host
validation only, runs without a GPU: each call returns before the entry's first HIP call (several entries clear an
output with hipMemsetAsync right after their first checks, so only the checks in front of that are exercised), and
`fake` is never dereferenced."""
import ctypes

from pytorch_sparse_amd import _native as nat

i64, vp, sz, ci = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
fake = vp(0x1000)
BIG = sz(1 << 40)
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 4
TWO31 = 1 << 31


def L():
    lib = nat.lib()
    for name in ('match', 'assign', 'conn', 'commit'):
        getattr(lib, 'tsamd_partition_%s_workspace_bytes' % name).restype = sz
    return lib


def edges(row=fake, col=fake, E=5, n=4, n_key=4, row_out=fake, col_out=fake, w_out=fake, info=fake):
    return L().tsamd_partition_edges(row, col, fake, None, i64(E), i64(n), i64(n_key), ci(1), row_out, col_out, w_out, info, None)


def vertex_weights(vw=fake, cmap=fake, n=4, n_c=2, out=fake):
    return L().tsamd_partition_vertex_weights(vw, cmap, i64(n), i64(n_c), out, None)


def match(rowptr=fake, vw=fake, n=4, rounds=4, match_=fake, cmap=fake, n_coarse=fake, ws=fake, wsb=BIG):
    return L().tsamd_partition_match(rowptr, fake, fake, vw, i64(n), i64(2), i64(rounds), match_, cmap, n_coarse, ws, wsb, None)


def bfs_init(n=4, state=fake):
    return L().tsamd_partition_bfs_init(fake, i64(n), fake, state, None)


def bfs_seed(cl=fake, n=4, comp=0, state=fake):
    return L().tsamd_partition_bfs_seed(cl, i64(n), i64(comp), ci(1), state, None)


def bfs_step(n=4, comp=0, level=0, state=fake):
    return L().tsamd_partition_bfs_step(fake, fake, i64(n), fake, i64(comp), i64(level), state, None)


def assign(cl=fake, vw=fake, n=4, k=2, part=fake, ws=fake, wsb=BIG):
    return L().tsamd_partition_assign(cl, vw, i64(n), i64(k), part, ws, wsb, None)


def part_weights(n=4, k=2, pw=fake):
    return L().tsamd_partition_part_weights(fake, fake, i64(n), i64(k), pw, None)


def conn(rowptr=fake, vw=fake, part=fake, pw=fake, n=4, k=2, mode=0, dest=fake, gain=fake, ws=fake, wsb=BIG):
    return L().tsamd_partition_conn(rowptr, fake, fake, vw, part, pw, i64(n), i64(k), i64(9), ci(mode), None, dest, gain, ws,
                                    wsb, None)


def recount(row=fake, col=fake, w=fake, part=fake, pw=fake, gain=fake, n=4, E=5, dest=fake, acc=fake):
    return L().tsamd_partition_recount(row, col, w, part, pw, gain, i64(n), i64(E), i64(9), dest, acc, None)


def commit(dest=fake, gain=fake, vw=fake, part=fake, pw=fake, n=4, k=2, ws=fake, wsb=BIG):
    return L().tsamd_partition_commit(dest, gain, vw, part, pw, i64(n), i64(k), i64(9), ci(0), ws, wsb, None)


def apply(dest=fake, vw=fake, n=4, k=2, part=fake, pw=fake, moved=fake):
    return L().tsamd_partition_apply(dest, vw, i64(n), i64(k), part, pw, moved, None)


def cut(E=5, out=fake):
    return L().tsamd_partition_cut(fake, fake, fake, fake, i64(E), out, None)


def keep_better(cuts=fake, over=fake, part_old=fake, pw_old=fake, n=4, k=2, part=fake, pw=fake):
    return L().tsamd_partition_keep_better(cuts, over, part_old, pw_old, i64(n), i64(k), part, pw, None)


def balance(pw=fake, k=2, out=fake):
    return L().tsamd_partition_balance(pw, i64(k), i64(9), out, None)


def test_negative_sizes_are_invalid():
    assert edges(E=-1) == edges(n=-1) == edges(n_key=-1) == INVALID
    assert vertex_weights(n=-1) == vertex_weights(n_c=-1) == INVALID
    assert match(n=-1) == match(rounds=-1) == INVALID
    assert bfs_init(n=-1) == bfs_seed(n=-1) == bfs_seed(comp=-1) == INVALID
    assert bfs_step(n=-1) == bfs_step(comp=-1) == bfs_step(level=-1) == INVALID
    assert assign(n=-1) == part_weights(n=-1) == conn(n=-1) == commit(n=-1) == apply(n=-1) == keep_better(n=-1) == INVALID
    assert recount(n=-1) == recount(E=-1) == cut(E=-1) == INVALID
    assert conn(mode=-1) == conn(mode=3) == INVALID


def test_fewer_than_one_part_is_invalid():
    for k in (0, -5):
        assert assign(k=k) == part_weights(k=k) == conn(k=k) == commit(k=k) == apply(k=k) == keep_better(k=k) == INVALID
        assert balance(k=k) == INVALID
        assert assign(k=k, n=0) == conn(k=k, n=0) == commit(k=k, n=0) == apply(k=k, n=0) == INVALID   # before "nothing to do"


def test_missing_pointers_are_invalid():
    assert edges(info=None) == edges(info=None, E=0) == INVALID
    for name in ('row', 'col', 'row_out', 'col_out', 'w_out'):
        assert edges(**{name: None}) == INVALID
    assert vertex_weights(out=None) == vertex_weights(vw=None) == vertex_weights(cmap=None) == INVALID
    assert match(n_coarse=None) == match(n_coarse=None, n=0) == INVALID
    assert match(rowptr=None) == match(vw=None) == match(match_=None) == match(cmap=None) == INVALID
    assert match(rowptr=None, ws=None, wsb=sz(0)) == INVALID   # a null pointer is reported first
    assert bfs_init(state=None) == bfs_seed(state=None) == bfs_seed(cl=None) == bfs_step(state=None) == INVALID
    assert assign(cl=None) == assign(vw=None) == assign(part=None) == INVALID
    assert part_weights(pw=None) == INVALID
    for name in ('rowptr', 'vw', 'part', 'pw', 'dest', 'gain'):
        assert conn(**{name: None}) == INVALID
    for name in ('row', 'col', 'w', 'part', 'pw', 'gain', 'dest', 'acc'):
        assert recount(**{name: None}) == INVALID
    for name in ('part', 'pw', 'gain', 'dest', 'acc'):
        assert recount(**{name: None, 'E': 0}) == INVALID
    for name in ('dest', 'gain', 'vw', 'part', 'pw'):
        assert commit(**{name: None}) == INVALID
    assert apply(moved=None) == apply(moved=None, n=0) == INVALID
    for name in ('dest', 'vw', 'part', 'pw'):
        assert apply(**{name: None}) == INVALID
    assert cut(out=None) == INVALID
    for name in ('cuts', 'over', 'pw_old', 'pw', 'part_old', 'part'):
        assert keep_better(**{name: None}) == INVALID
    assert keep_better(cuts=None, n=0) == keep_better(pw=None, n=0) == INVALID
    assert balance(pw=None) == balance(out=None) == INVALID


def test_two_to_the_31_is_unsupported():
    assert match(n=TWO31) == match(n=TWO31 + 5) == UNSUPPORTED and match(n=TWO31, n_coarse=None) == INVALID
    assert bfs_init(n=TWO31) == UNSUPPORTED and bfs_init(n=TWO31, state=None) == INVALID
    assert conn(k=TWO31) == conn(k=TWO31, n=0) == UNSUPPORTED and conn(k=TWO31, mode=3) == INVALID


def test_a_short_workspace():
    lib = L()
    for n, k in ((4, 2), (100000, 301)):
        need = {'match': lib.tsamd_partition_match_workspace_bytes(i64(n)),
                'assign': lib.tsamd_partition_assign_workspace_bytes(i64(n)),
                'conn': lib.tsamd_partition_conn_workspace_bytes(i64(n), i64(k)),
                'commit': lib.tsamd_partition_commit_workspace_bytes(i64(n), i64(k))}
        assert need['conn'] >= 8 * (n + 64 * k) and need['commit'] >= 8 * 7 * n and need['match'] >= 16 * n
        for f, key, kw in ((match, 'match', {}), (assign, 'assign', {'k': k}), (conn, 'conn', {'k': k}),
                           (commit, 'commit', {'k': k})):
            assert f(n=n, ws=None, **kw) == WORKSPACE and f(n=n, wsb=sz(0), **kw) == WORKSPACE
            assert f(n=n, wsb=sz(need[key] - 1), **kw) == WORKSPACE


def test_nothing_to_do_is_ok():
    assert edges(E=0) == edges(E=0, row=None, col=None, row_out=None, col_out=None, w_out=None) == OK
    assert vertex_weights(n_c=0) == vertex_weights(n_c=0, vw=None, cmap=None, out=None) == OK
    assert assign(n=0) == assign(n=0, cl=None, vw=None, part=None, ws=None, wsb=sz(0)) == OK
    assert conn(n=0) == conn(n=0, rowptr=None, vw=None, part=None, pw=None, dest=None, gain=None, ws=None, wsb=sz(0)) == OK
    assert recount(n=0) == commit(n=0) == commit(n=0, dest=None, ws=None, wsb=sz(0)) == apply(n=0) == OK
