"""hgt_sample (HGT budget sampling, the operator behind HGTLoader) on one MI355X.  Graph: the three node types
(2^20 / 2^19 / 2^10) and five relations of the hetero sampler rows of scripts/bench_sample.py, degrees 0..39, made
hub-heavy: 1 % of the columns hold 51..5000 entries (heavy tail).  Wall time of the op including its host read-backs,
median of 7 after 2 warm-up calls.  The reference has this op on the CPU only and oracle/_ref does not build it: GPU
numbers only.  Prints one JSON object per line:
  bench = hgt_sample             one row per (inputs, num_samples per type and hop, hops):
      nodes / edges   output sizes; winners = nodes drawn per hop, candidates = live budget entries a hop drew from
                      (all types together; measured by letting a last hop take the whole budget under the same seed)
      syncs           host read-backs of one call (torch's sync debug mode warns on each)
  bench = hetero_neighbor_sample the uniform sampler on the same graph, for scale
  bench = tsamd_hgt_select       the selection alone through the C-ABI: C candidates with random budgets, k winners
                                 (the rows with C just above k: what a radix-select route would still have to sort)
With --profile: a few calls of one configuration and nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pytorch_sparse_amd  # noqa: E402,F401
from pytorch_sparse_amd import _native as nat  # noqa: E402

dev = torch.device('cuda:0')
hgt = torch.ops.torch_sparse.hgt_sample


def wall(fn, iters=7, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return t[len(t) // 2] * 1e3


def count_syncs(fn):
    import tempfile
    torch.cuda.synchronize()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode='w+b') as tmp:
        os.dup2(tmp.fileno(), 2)
        torch.cuda.set_sync_debug_mode('warn')
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode('default')
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode(errors='replace').count('called a synchronizing')


scale = int(os.environ.get('SCALE', 20))
NODE_TYPES = ['paper', 'author', 'venue']
EDGE_TYPES = [('author', 'writes', 'paper'), ('paper', 'cites', 'paper'), ('paper', 'in', 'venue'),
              ('venue', 'hosts', 'paper'), ('paper', 'by', 'author')]
RELS = ['__'.join(e) for e in EDGE_TYPES]
sizes = {'paper': 1 << scale, 'author': 1 << (scale - 1), 'venue': 1 << 10}
gh = torch.Generator(device=dev).manual_seed(1)
colptr_d, row_d = {}, {}
for (s_, r_, d_) in EDGE_TYPES:
    deg = torch.randint(0, 40, (sizes[d_], ), generator=gh, device=dev)
    u = torch.rand(sizes[d_], generator=gh, device=dev)
    hub = torch.rand(sizes[d_], generator=gh, device=dev) < 0.01
    deg = torch.where(hub, (51.0 / (1.0 - 0.99 * u)).long().clamp(max=5000), deg)
    cp = torch.zeros(sizes[d_] + 1, dtype=torch.long, device=dev)
    cp[1:] = deg.cumsum(0)
    colptr_d['__'.join((s_, r_, d_))] = cp
    row_d['__'.join((s_, r_, d_))] = torch.randint(0, sizes[s_], (int(cp[-1]), ), generator=gh, device=dev)
perm = torch.randperm(sizes['paper'], generator=torch.Generator().manual_seed(0)).to(dev)


def hgt_row(inputs, k, hops):
    inp = {'paper': perm[:inputs]}
    ns = {t: [k] * hops for t in NODE_TYPES}
    fn = lambda: hgt(colptr_d, row_d, inp, ns, hops)  # noqa: E731
    ms = wall(fn)
    torch.manual_seed(0)
    node, r, c, e = fn()
    winners, cands, before = [], [], inputs
    for hop in range(hops):
        # the same call cut after `hop`, its last hop taking whatever the budgets hold: the live candidates of that hop
        torch.manual_seed(0)
        cut = hgt(colptr_d, row_d, inp, {t: [k] * hop + [1 << 40] for t in NODE_TYPES}, hop + 1)[0]
        torch.manual_seed(0)
        upto = hgt(colptr_d, row_d, inp, {t: [k] * (hop + 1) for t in NODE_TYPES}, hop + 1)[0]
        n_upto = sum(v.numel() for v in upto.values())
        cands.append(sum(v.numel() for v in cut.values()) - before)
        winners.append(n_upto - before)
        before = n_upto
    print(json.dumps(dict(bench='hgt_sample', inputs=inputs, num_samples=k, hops=hops, relations=len(RELS), ms=round(ms, 3),
                          nodes=sum(v.numel() for v in node.values()), edges=sum(v.numel() for v in e.values()),
                          winners=winners, candidates=cands, syncs=count_syncs(fn))), flush=True)


def select_row(C, k, M=1 << 20):
    L = nat.lib()
    L.tsamd_hgt_select_workspace_bytes.restype = ctypes.c_size_t
    g = torch.Generator(device=dev).manual_seed(C)
    cand = torch.randperm(M, generator=g, device=dev)[:C].contiguous()
    budget = torch.randint(1, 1 << 34, (C, ), generator=g, device=dev)
    ws = torch.empty(L.tsamd_hgt_select_workspace_bytes(ctypes.c_int64(C)), dtype=torch.uint8, device=dev)
    out = torch.empty(k, dtype=torch.long, device=dev)
    err = torch.zeros(1, dtype=torch.long, device=dev)
    word = torch.zeros(M, dtype=torch.long, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    I = lambda x: ctypes.c_int64(int(x))  # noqa: E731
    st = nat.stream_ptr(dev)
    reps = 20

    def fn():
        for i in range(reps):
            word[cand] = budget  # (the winners of the call before turned seen)
            nat.check(L.tsamd_hgt_select(P(cand), I(C), P(word), I(M), I(k), ctypes.c_uint64(i), I(0), I(0), P(out), P(err),
                                         P(ws), ctypes.c_size_t(ws.numel()), st), 'tsamd_hgt_select')

    def fill_only():
        for i in range(reps):
            word[cand] = budget

    us = (wall(fn) - wall(fill_only)) / reps * 1e3
    assert int(err.item()) == 0 and int(out.min()) >= 0
    print(json.dumps(dict(bench='tsamd_hgt_select', route='a (keys + one radix sort of all candidates)', candidates=C, k=k,
                          us=round(us, 1))), flush=True)


if '--profile' in sys.argv:
    inp = {'paper': perm[:1024]}
    ns = {t: [2048] * 4 for t in NODE_TYPES}
    for _ in range(12):
        hgt(colptr_d, row_d, inp, ns, 4)
    torch.cuda.synchronize()
    sys.exit(0)

for inputs in (128, 1024):
    for k in (512, 2048):
        for hops in (2, 4):
            hgt_row(inputs, k, hops)
for inputs, fanv, hops in ((128, 10, 2), (1024, 10, 2), (1024, 5, 4)):
    inp_d = {'paper': perm[:inputs]}
    fan_d = {r: [fanv] * hops for r in RELS}
    fn = lambda: torch.ops.torch_sparse.hetero_neighbor_sample(NODE_TYPES, EDGE_TYPES, colptr_d, row_d, inp_d, fan_d, hops,  # noqa: E731
                                                               False, True)
    ms = wall(fn)
    out = fn()
    print(json.dumps(dict(bench='hetero_neighbor_sample', inputs=inputs, fanout=fanv, hops=hops, relations=len(RELS),
                          ms=round(ms, 3), nodes=sum(out[0][t].numel() for t in NODE_TYPES),
                          edges=sum(out[3][r].numel() for r in RELS), syncs=count_syncs(fn))), flush=True)
for C in (10000, 100000, 1000000):
    for k in (512, 2048):
        select_row(C, k)
# the floor of a radix-select route (b): its final sort of the ~k candidates at or below the threshold bin alone
select_row(600, 512)
select_row(2200, 2048)
