// torch_sparse::partition / partition2 / mt_partition (reference schemas, csrc/metis.cpp:18-69) on device tensors: the
// host driver of the multilevel k-way partitioner of csrc/partition.hip, plus tsamd::partition_match / _contract /
// _initial / _refine, which run one phase on explicit inputs (tests/test_partition_gpu.py).  docs/design/partition.md
// describes the scheme.  No graph array crosses to the host; what the driver reads back are sizes and flags:
//   level 0            1 read   (entries of A + A^T, weight sums, range errors, vertex-weight sum / min / max)
//   coarsening         1 read per level   (coarse vertices, coarse entries, parked self-loops)
//   initial partition  1 read per BFS level and per component of the coarsest graph   (frontier grew / seed found)
//   refinement         1 read per round   (vertices moved), 1 per rebalance pass   (parts over capacity, moved)
#include "ops_common.h"

#include <chrono>

namespace tsamd_ops {
namespace {

constexpr int64_t kCoarsenPerPart = 64, kCoarsenFloor = 512, kMatchRounds = 4, kRefineRounds = 8, kMaxLevels = 64;

struct Graph {
  Tensor rowptr, row, col, w, vw;
  int64_t n = 0, E = 0;
};

inline int64_t *lp(const Tensor &t) { return t.data_ptr<int64_t>(); }
inline Tensor i64_empty(int64_t n, const Tensor &like) { return torch::empty({n}, like.options().dtype(at::kLong)); }
inline Tensor i64_zeros(int64_t n, const Tensor &like) { return torch::zeros({n}, like.options().dtype(at::kLong)); }
inline std::vector<int64_t> read_back(const Tensor &t) {  // the driver's only kind of host sync
  const Tensor h = t.cpu();
  return std::vector<int64_t>(h.data_ptr<int64_t>(), h.data_ptr<int64_t>() + h.numel());
}

// the level built from an entry list: (cmap[row], cmap[col], w) [+ transposes], self-loops dropped, duplicates summed.
// info = int64[8] on the device: [0..3] tsamd_partition_edges, [4] the level's vertex count when it is only known there
// (n_out < 0), [5..7] the counts of the coalesce.  One read-back.  -> (graph without vw, host copy of info)
std::pair<Graph, std::vector<int64_t>> build_level(const Tensor &row, const Tensor &col, const OptTensor &w,
                                                   const OptTensor &cmap, int64_t n, int64_t n_out, bool mirror,
                                                   Tensor info, const OptTensor &extra) {
  void *stream = current_stream(row);
  const int64_t E = row.numel(), L = mirror ? 2 * E : E;
  Tensor r = i64_empty(L, row), c = i64_empty(L, row), x = i64_empty(L, row);
  check_status(tsamd_partition_edges(lp(row), lp(col), w.has_value() ? lp(w.value()) : nullptr,
                                     cmap.has_value() ? lp(cmap.value()) : nullptr, E, n, n, mirror ? 1 : 0, lp(r), lp(c),
                                     lp(x), lp(info), stream),
               "tsamd_partition_edges");
  Tensor row_t = i64_empty(L, row), col_t = i64_empty(L, row), row_u = i64_empty(L, row), col_u = i64_empty(L, row);
  Tensor seg = i64_empty(L + 1, row), x_s = i64_empty(L, row);
  if (L > 0) {
    Tensor ws = workspace(tsamd_sort_coalesce_workspace_bytes(L), row);
    check_status(tsamd_sort_coalesce(lp(r), lp(c), L, n + 1, n > 0 ? n : 1, lp(row_t), lp(col_t), lp(row_u), lp(col_u),
                                     lp(seg), lp(info) + 5, lp(x), lp(x_s), 8, ws.data_ptr(), (size_t)ws.numel(), stream),
                 "tsamd_sort_coalesce");
  }
  std::vector<int64_t> host = read_back(extra.has_value() ? torch::cat({info, extra.value()}) : info);
  const int64_t distinct = L > 0 ? host[7] : 0, nnz = distinct - (host[3] > 0 ? 1 : 0);  // the parked key sorts last
  Graph g;
  g.n = n_out >= 0 ? n_out : host[4];
  g.E = nnz;
  Tensor w_u = i64_empty(distinct, row);
  if (distinct > 0)
    check_status(tsamd_segment_reduce(TSAMD_I64, TSAMD_SUM, x_s.data_ptr(), nullptr, lp(seg), distinct, 1, w_u.data_ptr(),
                                      stream),
                 "tsamd_segment_reduce");
  g.row = row_u.narrow(0, 0, nnz);
  g.col = col_u.narrow(0, 0, nnz);
  g.w = w_u.narrow(0, 0, nnz);
  g.rowptr = i64_empty(g.n + 1, row);
  check_status(tsamd_ind2ptr(lp(g.row), g.n, nnz, lp(g.rowptr), stream), "tsamd_ind2ptr");
  return {g, host};
}

// matching of one level -> (match, cmap), the number of coarse vertices in n_coarse[0] on the device
std::pair<Tensor, Tensor> match_level(const Graph &g, int64_t cap, int64_t rounds, int64_t *n_coarse) {
  Tensor match = i64_empty(g.n, g.rowptr), cmap = i64_empty(g.n, g.rowptr);
  Tensor ws = workspace(tsamd_partition_match_workspace_bytes(g.n), g.rowptr);
  check_status(tsamd_partition_match(lp(g.rowptr), lp(g.col), lp(g.w), lp(g.vw), g.n, cap, rounds, lp(match), lp(cmap),
                                     n_coarse, ws.data_ptr(), (size_t)ws.numel(), current_stream(g.rowptr)),
               "tsamd_partition_match");
  return {match, cmap};
}

Tensor coarse_vertex_weights(const Tensor &vw, const Tensor &cmap, int64_t n_c) {
  Tensor out = i64_empty(n_c, vw);
  check_status(tsamd_partition_vertex_weights(lp(vw), lp(cmap), vw.numel(), n_c, lp(out), current_stream(vw)),
               "tsamd_partition_vertex_weights");
  return out;
}

Tensor initial_partition(const Graph &g, int64_t k) {
  void *stream = current_stream(g.rowptr);
  Tensor cl = i64_empty(g.n, g.rowptr), state = i64_empty(4, g.rowptr), part = i64_empty(g.n, g.rowptr);
  check_status(tsamd_partition_bfs_init(lp(g.rowptr), g.n, lp(cl), lp(state), stream), "tsamd_partition_bfs_init");
  for (int64_t comp = 0; comp <= g.n; ++comp) {
    check_status(tsamd_partition_bfs_seed(lp(cl), g.n, comp, comp == 0, lp(state), stream), "tsamd_partition_bfs_seed");
    if (read_back(state)[2] == 0) break;  // every vertex has been visited
    for (int64_t level = 0; level <= g.n; ++level) {
      check_status(tsamd_partition_bfs_step(lp(g.rowptr), lp(g.col), g.n, lp(cl), comp, level, lp(state), stream),
                   "tsamd_partition_bfs_step");
      if (read_back(state)[3] == 0) break;  // the frontier is empty
    }
  }
  Tensor ws = workspace(tsamd_partition_assign_workspace_bytes(g.n), g.rowptr);
  check_status(tsamd_partition_assign(lp(cl), lp(g.vw), g.n, k, lp(part), ws.data_ptr(), (size_t)ws.numel(), stream),
               "tsamd_partition_assign");
  return part;
}

// refinement rounds + rebalance on one level, in place on `part`.  first (nullable): receives the destinations and gains
// the connectivity kernels report in round 0.
void refine_level(const Graph &g, Tensor &part, int64_t k, int64_t cap, int64_t rounds, std::pair<Tensor, Tensor> *first) {
  void *stream = current_stream(g.rowptr);
  const int64_t n = g.n;
  Tensor pw = i64_empty(k, part), pw_old = i64_empty(k, part), part_old = i64_empty(n, part);
  Tensor dest = i64_empty(n, part), gain = i64_empty(n, part), acc = i64_empty(n, part);
  Tensor st = i64_zeros(8, part);  // [0..1] cuts, [2..4] balance, [5] moved
  int64_t *cuts = lp(st), *bal = lp(st) + 2, *moved = lp(st) + 5;
  Tensor conn_ws = workspace(tsamd_partition_conn_workspace_bytes(n, k), part);
  Tensor commit_ws = workspace(tsamd_partition_commit_workspace_bytes(n, k), part);
  check_status(tsamd_partition_part_weights(lp(part), lp(g.vw), n, k, lp(pw), stream), "tsamd_partition_part_weights");
  check_status(tsamd_partition_cut(lp(g.row), lp(g.col), lp(g.w), lp(part), g.E, cuts, stream), "tsamd_partition_cut");
  auto conn = [&](int mode, const int64_t *lightest) {
    check_status(tsamd_partition_conn(lp(g.rowptr), lp(g.col), lp(g.w), lp(g.vw), lp(part), lp(pw), n, k, cap, mode,
                                      lightest, lp(dest), lp(gain), conn_ws.data_ptr(), (size_t)conn_ws.numel(), stream),
                 "tsamd_partition_conn");
  };
  auto commit = [&](int select) {
    check_status(tsamd_partition_commit(lp(dest), lp(gain), lp(g.vw), lp(part), lp(pw), n, k, cap, select,
                                        commit_ws.data_ptr(), (size_t)commit_ws.numel(), stream),
                 "tsamd_partition_commit");
  };
  auto apply = [&]() {
    st.narrow(0, 5, 1).zero_();
    check_status(tsamd_partition_apply(lp(dest), lp(g.vw), n, k, lp(part), lp(pw), moved, stream), "tsamd_partition_apply");
  };
  int idle = 0;
  for (int64_t round = 0; round < rounds && idle < 2; ++round) {
    check_status(tsamd_partition_balance(lp(pw), k, cap, bal, stream), "tsamd_partition_balance");
    conn((int)(round & 1), nullptr);
    if (round == 0 && first) *first = {dest.clone(), gain.clone()};
    check_status(tsamd_partition_recount(lp(g.row), lp(g.col), lp(g.w), lp(part), lp(pw), lp(gain), n, g.E, cap, lp(dest),
                                         lp(acc), stream),
                 "tsamd_partition_recount");
    commit(0);
    part_old.copy_(part);
    pw_old.copy_(pw);
    apply();
    check_status(tsamd_partition_cut(lp(g.row), lp(g.col), lp(g.w), lp(part), g.E, cuts + 1, stream), "tsamd_partition_cut");
    check_status(tsamd_partition_keep_better(cuts, bal, lp(part_old), lp(pw_old), n, k, lp(part), lp(pw), stream),
                 "tsamd_partition_keep_better");
    idle = read_back(st)[5] == 0 ? idle + 1 : 0;
  }
  // rebalance: while a part is over capacity, its lowest-loss vertices move to a part with room
  for (int64_t pass = 0; pass < 4 * k + 16; ++pass) {
    check_status(tsamd_partition_balance(lp(pw), k, cap, bal, stream), "tsamd_partition_balance");
    const std::vector<int64_t> h = read_back(st);
    if (h[2] == 0 || (pass > 0 && h[5] == 0)) break;
    conn(2, bal + 2);
    commit(1);
    commit(0);
    apply();
  }
}

void project(const Tensor &part_c, const Tensor &cmap, Tensor &part) {
  check_status(tsamd_gather_rows(part_c.data_ptr(), lp(cmap), part.data_ptr(), cmap.numel(), part_c.numel(), 8,
                                 current_stream(cmap)),
               "tsamd_gather_rows");
}

void check_graph_args(const Tensor &rowptr, const Tensor &col) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  TORCH_CHECK(rowptr.numel() >= 1, "rowptr must have at least one entry");
  TORCH_CHECK(col.numel() < ((int64_t)1 << 31) && rowptr.numel() <= ((int64_t)1 << 31),
              "partition: at most 2^31 - 1 vertices and entries");
}

Tensor weights_arg(const OptTensor &t, int64_t numel, const char *name, const Tensor &like) {
  if (!t.has_value()) return torch::ones({numel}, like.options().dtype(at::kLong));
  check_gpu(t.value(), name);
  TORCH_CHECK(t.value().numel() == numel, name, " has the wrong number of elements");
  TORCH_CHECK(at::isIntegralType(t.value().scalar_type(), false), name, " must be an integer tensor (weight2metis)");
  return t.value().reshape({-1}).to(at::kLong).contiguous();
}

// phase_ms (nullable): wall milliseconds of (level 0, coarsening, initial partition, refinement), each closed by a
// stream synchronisation that an untimed call does not make
struct PhaseClock {
  double *ms;
  void *stream;
  std::chrono::steady_clock::time_point t0;
  PhaseClock(double *ms_, void *stream_) : ms(ms_), stream(stream_), t0(std::chrono::steady_clock::now()) {}
  void lap(int phase) {
    if (!ms) return;
    (void)hipStreamSynchronize((hipStream_t)stream);
    const auto t1 = std::chrono::steady_clock::now();
    ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

Tensor partition_impl(const Tensor &rowptr_, const Tensor &col_, const OptTensor &opt_value, const OptTensor &opt_nw,
                      int64_t k, bool recursive, double *phase_ms = nullptr) {
  (void)recursive;  // the k-way scheme serves both (documented divergence)
  if (!rowptr_.device().is_cuda()) TORCH_CHECK(false, "Not compiled with METIS support");
  check_graph_args(rowptr_, col_);
  TORCH_CHECK(k >= 1 && k < ((int64_t)1 << 31), "partition: num_parts must be in [1, 2^31)");
  c10::hip::HIPGuard guard(rowptr_.get_device());
  const Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous();
  void *stream = current_stream(rowptr);
  const int64_t n = rowptr.numel() - 1, E = col.numel();
  if (n == 0 || k == 1) return i64_zeros(n, rowptr);
  PhaseClock clock(phase_ms, stream);
  OptTensor value;
  if (opt_value.has_value()) value = weights_arg(opt_value, E, "value", rowptr);
  const Tensor vw = weights_arg(opt_nw, n, "node_weight", rowptr);

  // vertex-weight sum / max / min with the entry-balanced segment reduction over ONE segment
  Tensor vstats = i64_empty(3, rowptr), seg01 = torch::tensor({(int64_t)0, n}, rowptr.options().dtype(at::kLong));
  {
    Tensor ws = workspace(tsamd_segment_reduce_balanced_workspace_bytes(TSAMD_I64, n, 1), rowptr);
    const int reds[3] = {TSAMD_SUM, TSAMD_MAX, TSAMD_MIN};
    for (int i = 0; i < 3; ++i)
      check_status(tsamd_segment_reduce_balanced(TSAMD_I64, reds[i], vw.data_ptr(), nullptr, lp(seg01), 1, n, 1,
                                                 lp(vstats) + i, ws.data_ptr(), (size_t)ws.numel(), stream),
                   "tsamd_segment_reduce_balanced");
  }
  Tensor row = i64_empty(E, rowptr);
  check_status(tsamd_ptr2ind(lp(rowptr), n, E, lp(row), stream), "tsamd_ptr2ind");
  auto built = build_level(row, col, value, c10::nullopt, n, n, true, i64_zeros(8, rowptr), vstats);
  Graph g = built.first;
  const std::vector<int64_t> &h = built.second;
  TORCH_CHECK(h[2] == 0, "partition: column ids must lie in [0, rows) and weights must not be negative");
  const int64_t W = h[8], wmax = h[9], wmin = h[10];
  TORCH_CHECK(wmin >= 0, "partition: node weights must not be negative");
  TORCH_CHECK((unsigned __int128)(uint64_t)h[0] + ((unsigned __int128)(uint64_t)h[1] << 32) < ((unsigned __int128)1 << 62),
              "partition: the total edge weight exceeds 2^62");
  TORCH_CHECK(W >= 0 && (unsigned __int128)W * 2 * (unsigned __int128)k < ((unsigned __int128)1 << 62),
              "partition: total node weight x num_parts exceeds 2^61");
  g.vw = vw;
  const int64_t cap = (int64_t)(((unsigned __int128)W * 103) / ((unsigned __int128)k * 100)) + wmax;
  const int64_t target = std::max(kCoarsenPerPart * k, kCoarsenFloor);
  const int64_t match_cap = std::max(wmax, (3 * W) / (2 * target));

  clock.lap(0);
  std::vector<Graph> levels{g};
  std::vector<Tensor> cmaps;
  while (levels.back().n > target && (int64_t)levels.size() < kMaxLevels) {
    const Graph &f = levels.back();
    Tensor info = i64_zeros(8, rowptr);
    auto mc = match_level(f, match_cap, kMatchRounds, lp(info) + 4);
    auto lvl = build_level(f.row, f.col, f.w, mc.second, f.n, -1, false, info, c10::nullopt);
    Graph c = lvl.first;
    if (c.n * 100 > f.n * 95) break;  // matching has stalled (hub-and-leaf stars): partition this level
    c.vw = coarse_vertex_weights(f.vw, mc.second, c.n);
    levels.push_back(c);
    cmaps.push_back(mc.second);
  }
  clock.lap(1);
  Tensor part = initial_partition(levels.back(), k);
  clock.lap(2);
  refine_level(levels.back(), part, k, cap, kRefineRounds, nullptr);
  for (int64_t l = (int64_t)levels.size() - 2; l >= 0; --l) {
    Tensor fine = i64_empty(levels[l].n, rowptr);
    project(part, cmaps[l], fine);
    part = fine;
    refine_level(levels[l], part, k, cap, kRefineRounds, nullptr);
  }
  clock.lap(3);
  return part;
}

// partition2 with the wall time of its phases (scripts/bench_partition.py) -> (cluster, [level 0, coarsening, initial
// partition, refinement] in milliseconds)
std::tuple<Tensor, std::vector<double>> partition_timed(Tensor rowptr, Tensor col, OptTensor optional_value,
                                                        OptTensor optional_node_weight, int64_t num_parts) {
  std::vector<double> ms(4, 0.0);
  Tensor part = partition_impl(rowptr, col, optional_value, optional_node_weight, num_parts, false, ms.data());
  return std::make_tuple(part, ms);
}

Tensor partition(Tensor rowptr, Tensor col, OptTensor optional_value, int64_t num_parts, bool recursive) {
  return partition_impl(rowptr, col, optional_value, c10::nullopt, num_parts, recursive);
}
Tensor partition2(Tensor rowptr, Tensor col, OptTensor optional_value, OptTensor optional_node_weight, int64_t num_parts,
                  bool recursive) {
  return partition_impl(rowptr, col, optional_value, optional_node_weight, num_parts, recursive);
}
Tensor mt_partition(Tensor rowptr, Tensor col, OptTensor optional_value, OptTensor optional_node_weight,
                    int64_t num_parts, bool recursive, int64_t num_workers) {
  (void)num_workers;
  return partition_impl(rowptr, col, optional_value, optional_node_weight, num_parts, recursive);
}

// ---- one phase on explicit inputs -----------------------------------------------------------------------------------
Graph graph_arg(const Tensor &rowptr, const Tensor &col, const OptTensor &weight, const Tensor &vweight) {
  check_graph_args(rowptr, col);
  Graph g;
  g.rowptr = rowptr.contiguous();
  g.col = col.contiguous();
  g.n = rowptr.numel() - 1;
  g.E = col.numel();
  g.w = weights_arg(weight, g.E, "weight", rowptr);
  g.vw = weights_arg(vweight, g.n, "vweight", rowptr);
  g.row = i64_empty(g.E, rowptr);
  check_status(tsamd_ptr2ind(lp(g.rowptr), g.n, g.E, lp(g.row), current_stream(rowptr)), "tsamd_ptr2ind");
  if (g.E > 0) {
    TORCH_CHECK(g.col.min().item<int64_t>() >= 0 && g.col.max().item<int64_t>() < g.n, "col out of range");
    TORCH_CHECK(g.w.min().item<int64_t>() >= 0, "negative weight");
  }
  return g;
}

// -> (match [n] partner or -1, cmap [n], number of coarse vertices [1])
std::tuple<Tensor, Tensor, Tensor> partition_match(Tensor rowptr, Tensor col, OptTensor weight, Tensor vweight, int64_t cap,
                                                   int64_t rounds) {
  c10::hip::HIPGuard guard(rowptr.get_device());
  const Graph g = graph_arg(rowptr, col, weight, vweight);
  Tensor n_c = i64_zeros(1, rowptr);
  auto mc = match_level(g, cap, rounds, lp(n_c));
  return std::make_tuple(mc.first, mc.second, n_c);
}

// -> (rowptr_c, col_c, weight_c, vweight_c) of the graph contracted along cmap (values in [0, n_c))
std::tuple<Tensor, Tensor, Tensor, Tensor> partition_contract(Tensor rowptr, Tensor col, OptTensor weight, Tensor vweight,
                                                              Tensor cmap, int64_t n_c) {
  c10::hip::HIPGuard guard(rowptr.get_device());
  const Graph g = graph_arg(rowptr, col, weight, vweight);
  check_index(cmap, "cmap");
  TORCH_CHECK(cmap.numel() == g.n && n_c >= 0, "cmap must have one entry per vertex");
  if (g.n > 0) TORCH_CHECK(cmap.min().item<int64_t>() >= 0 && cmap.max().item<int64_t>() < n_c, "cmap out of range");
  const Tensor cm = cmap.contiguous();
  auto lvl = build_level(g.row, g.col, g.w, cm, g.n, n_c, false, i64_zeros(8, rowptr), c10::nullopt);
  return std::make_tuple(lvl.first.rowptr, lvl.first.col.clone(), lvl.first.w.clone(), coarse_vertex_weights(g.vw, cm, n_c));
}

Tensor partition_initial(Tensor rowptr, Tensor col, Tensor vweight, int64_t k) {
  c10::hip::HIPGuard guard(rowptr.get_device());
  const Graph g = graph_arg(rowptr, col, c10::nullopt, vweight);
  TORCH_CHECK(k >= 1 && k < ((int64_t)1 << 31), "k must be in [1, 2^31)");
  return initial_partition(g, k);
}

// -> (part after `rounds` refinement rounds + rebalance, destination [n] and gain [n] reported in round 0)
std::tuple<Tensor, Tensor, Tensor> partition_refine(Tensor rowptr, Tensor col, OptTensor weight, Tensor vweight, Tensor part,
                                                    int64_t k, int64_t cap, int64_t rounds) {
  c10::hip::HIPGuard guard(rowptr.get_device());
  const Graph g = graph_arg(rowptr, col, weight, vweight);
  check_index(part, "part");
  TORCH_CHECK(k >= 1 && k < ((int64_t)1 << 31), "k must be in [1, 2^31)");
  TORCH_CHECK(part.numel() == g.n, "part must have one entry per vertex");
  if (g.n > 0) TORCH_CHECK(part.min().item<int64_t>() >= 0 && part.max().item<int64_t>() < k, "part out of range");
  Tensor p = part.clone().contiguous();
  std::pair<Tensor, Tensor> first{i64_empty(0, rowptr), i64_empty(0, rowptr)};
  refine_level(g, p, k, cap, rounds, &first);
  return std::make_tuple(p, first.first, first.second);
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_partition = torch::RegisterOperators()
                                     .op("torch_sparse::partition", &partition)
                                     .op("torch_sparse::partition2", &partition2)
                                     .op("torch_sparse::mt_partition", &mt_partition)
                                     .op("tsamd::partition_timed", &partition_timed)
                                     .op("tsamd::partition_match", &partition_match)
                                     .op("tsamd::partition_contract", &partition_contract)
                                     .op("tsamd::partition_initial", &partition_initial)
                                     .op("tsamd::partition_refine", &partition_refine);
