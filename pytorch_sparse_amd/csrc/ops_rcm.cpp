// tsamd::rcm / rcm_degree / rcm_limits (and the bench handle tsamd::rcm_tuned) on device tensors: the host driver of the reverse Cuthill-McKee ordering of
// csrc/rcm.hip (the reference calls scipy on the host, torch_sparse/bandwidth.py:8-20).  docs/design/rcm.md describes
// the scheme.  No graph array crosses to the host; what the driver reads back is the 8-word state record:
//   one-workgroup launch   1 read   (frontier bounds, seed cursor, why it stopped, input errors)
//   whole-device level     1 read   (entries of the frontier's rows, which size the level's launches)
// The prologue builds the working graph with the existing sort: nodes ranked by (degree, id) with one tsamd_sort_coo,
// the entries relabelled by rank and re-sorted with another -- the path behind select.permute.
#include "ops_common.h"

namespace tsamd_ops {
namespace {

constexpr int64_t kStateWords = 8;
enum { kLo = 0, kHi, kCursor, kReason, kLevels, kComponents, kEntries, kError };
enum { kDone = 0, kOver = 1, kBudget = 2, kSeedBudget = 3 };

inline int64_t *lp(const Tensor &t) { return t.data_ptr<int64_t>(); }
inline Tensor i64_empty(int64_t n, const Tensor &like) { return torch::empty({n}, like.options().dtype(at::kLong)); }

std::vector<int64_t> limits() {
  int64_t out[3];
  check_status(tsamd_rcm_limits(out), "tsamd_rcm_limits");
  return {out[0], out[1], out[2]};
}

void check_graph_args(const Tensor &rowptr, const Tensor &col) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  TORCH_CHECK(rowptr.numel() >= 1, "rowptr must have at least one entry");
  TORCH_CHECK(col.numel() < ((int64_t)1 << 31) && rowptr.numel() <= ((int64_t)1 << 31),
              "rcm: at most 2^31 - 1 nodes and entries");
}

Tensor degree_of(const Tensor &rowptr, const Tensor &col) {
  const int64_t n = rowptr.numel() - 1;
  Tensor deg = i64_empty(n, rowptr);
  check_status(tsamd_rcm_degree(lp(rowptr), lp(col), n, col.numel(), lp(deg), current_stream(rowptr)), "tsamd_rcm_degree");
  return deg;
}

// stable sort of (row, col) pairs with the existing radix sort -> (row_s, col_s)
std::pair<Tensor, Tensor> sort_pairs(const Tensor &row, const Tensor &col, int64_t M, int64_t N) {
  const int64_t E = row.numel();
  Tensor row_s = i64_empty(E, row), col_s = i64_empty(E, row), perm = i64_empty(E, row);
  if (E > 0) {
    Tensor ws = workspace(tsamd_sort_coo_workspace_bytes(E), row);
    check_status(tsamd_sort_coo(lp(row), lp(col), E, M, N, lp(row_s), lp(col_s), lp(perm), ws.data_ptr(),
                                (size_t)ws.numel(), current_stream(row)),
                 "tsamd_sort_coo");
  }
  return {row_s, col_s};
}

Tensor rcm_degree(Tensor rowptr, Tensor col) {
  check_graph_args(rowptr, col);
  c10::hip::HIPGuard guard(rowptr.get_device());
  return degree_of(rowptr.contiguous(), col.contiguous());
}

// -> (perm, stats = [levels, components, big_levels, small_launches, host_syncs]).  budget <= 0: the shipped one.
std::tuple<Tensor, Tensor> rcm_impl(const Tensor &rowptr_, const Tensor &col_, const Tensor &seeds_, int64_t small_cap,
                                    int64_t budget) {
  check_graph_args(rowptr_, col_);
  check_index(seeds_, "seed_order");
  const int64_t n = rowptr_.numel() - 1, E = col_.numel();
  TORCH_CHECK(seeds_.numel() == n, "seed_order must have one entry per node");
  c10::hip::HIPGuard guard(rowptr_.get_device());
  const Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous(), seeds = seeds_.contiguous();
  void *stream = current_stream(rowptr);
  const std::vector<int64_t> lim = limits();
  const int64_t cap = small_cap < 0 ? lim[0] : std::min(small_cap, lim[0]);
  if (budget <= 0) budget = lim[2];
  int64_t big_levels = 0, small_launches = 0, host_syncs = 0;
  auto stats = [&](int64_t levels, int64_t components) {
    return torch::tensor({levels, components, big_levels, small_launches, host_syncs}, torch::dtype(at::kLong));
  };
  Tensor perm = i64_empty(n, rowptr);
  if (n == 0) return std::make_tuple(perm, stats(0, 0));

  // prologue: by_rank = the nodes in stable (degree, id) order; the working graph = the entries relabelled by rank and
  // sorted by (row, col)
  Tensor state = torch::zeros({kStateWords}, rowptr.options().dtype(at::kLong));
  const Tensor deg = degree_of(rowptr, col);
  const Tensor by_rank = sort_pairs(deg, torch::arange(n, rowptr.options().dtype(at::kLong)), E + 2, n).second;
  Tensor rank = i64_empty(n, rowptr), seeds_r = i64_empty(n, rowptr), pos = i64_empty(n, rowptr);
  Tensor owner = i64_empty(n, rowptr), order = i64_empty(n, rowptr), fptr = i64_empty(n + 1, rowptr);
  check_status(tsamd_rcm_begin(lp(by_rank), lp(seeds), n, lp(rank), lp(seeds_r), lp(pos), lp(owner), lp(fptr), lp(state),
                               stream),
               "tsamd_rcm_begin");
  Tensor row = i64_empty(E, rowptr), row_r = i64_empty(E, rowptr), col_r = i64_empty(E, rowptr);
  if (E > 0) check_status(tsamd_ptr2ind(lp(rowptr), n, E, lp(row), stream), "tsamd_ptr2ind");
  check_status(tsamd_rcm_relabel(lp(row), lp(rank), E, n, lp(row_r), lp(state), stream), "tsamd_rcm_relabel");
  check_status(tsamd_rcm_relabel(lp(col), lp(rank), E, n, lp(col_r), lp(state), stream), "tsamd_rcm_relabel");
  auto sorted = sort_pairs(row_r, col_r, n, n);
  const Tensor wcol = sorted.second;
  Tensor wptr = i64_empty(n + 1, rowptr);
  check_status(tsamd_ind2ptr(lp(sorted.first), n, E, lp(wptr), stream), "tsamd_ind2ptr");
  row = row_r = col_r = Tensor();

  // the level loop: one-workgroup launches while the frontier fits, whole-device levels while it does not
  Tensor ej, ep, off, level_ws;
  auto read_state = [&]() {
    ++host_syncs;
    const Tensor h = state.cpu();
    const std::vector<int64_t> s(h.data_ptr<int64_t>(), h.data_ptr<int64_t>() + kStateWords);
    TORCH_CHECK(s[kError] != 1, "rcm: col holds an id outside [0, rows)");
    TORCH_CHECK(s[kError] == 0, "rcm: seed_order is not a permutation of the nodes");
    return s;
  };
  std::vector<int64_t> s;
  for (int64_t launch = 0;; ++launch) {
    TORCH_CHECK(launch <= 2 * n + 16, "rcm: the search does not advance");  // every launch orders a node or ends a route
    check_status(tsamd_rcm_small(lp(wptr), lp(wcol), lp(seeds_r), n, cap, budget, lp(pos), lp(owner), lp(order), lp(state),
                                 stream),
                 "tsamd_rcm_small");
    ++small_launches;
    s = read_state();
    if (s[kReason] == kDone) break;
    if (s[kReason] != kOver) continue;
    const int64_t nf = s[kHi] - s[kLo];
    TORCH_CHECK(nf > 0 && s[kHi] <= n, "rcm: inconsistent state record");
    if (!ej.defined()) {
      ej = i64_empty(E, rowptr);
      ep = i64_empty(E, rowptr);
      off = i64_empty(E, rowptr);
      level_ws = workspace(tsamd_rcm_level_workspace_bytes(std::max(E, n)), rowptr);
    }
    check_status(tsamd_rcm_level_plan(lp(wptr), lp(order), nf, lp(fptr), lp(state), level_ws.data_ptr(),
                                      (size_t)level_ws.numel(), stream),
                 "tsamd_rcm_level_plan");
    const int64_t T = read_state()[kEntries];
    TORCH_CHECK(T >= 0 && T <= E, "rcm: rowptr does not describe col");
    check_status(tsamd_rcm_level_run(lp(wptr), lp(wcol), lp(fptr), T, n, lp(pos), lp(owner), lp(order), lp(ej), lp(ep),
                                     lp(off), lp(state), level_ws.data_ptr(), (size_t)level_ws.numel(), stream),
                 "tsamd_rcm_level_run");
    ++big_levels;
  }
  TORCH_CHECK(s[kHi] == n, "rcm: the search ended with nodes left over");
  check_status(tsamd_rcm_finish(lp(order), lp(by_rank), n, lp(perm), stream), "tsamd_rcm_finish");
  return std::make_tuple(perm, stats(s[kLevels], s[kComponents]));
}

std::tuple<Tensor, Tensor> rcm(Tensor rowptr, Tensor col, Tensor seed_order, int64_t small_cap) {
  return rcm_impl(rowptr, col, seed_order, small_cap, 0);
}
// A bench and test handle, not part of the public surface: the same with the level budget of a one-workgroup launch
// chosen by the caller.  Only scripts/bench_rcm.py --sweep, the runs behind the shipped limits, calls it.
std::tuple<Tensor, Tensor> rcm_tuned(Tensor rowptr, Tensor col, Tensor seed_order, int64_t small_cap, int64_t budget) {
  TORCH_CHECK(budget >= 1 && budget <= ((int64_t)1 << 20), "rcm_tuned: budget must be in [1, 2^20]");
  return rcm_impl(rowptr, col, seed_order, small_cap, budget);
}

std::vector<int64_t> rcm_limits() { return limits(); }

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_rcm = torch::RegisterOperators()
                               .op("tsamd::rcm_degree", &rcm_degree)
                               .op("tsamd::rcm", &rcm)
                               .op("tsamd::rcm_tuned", &rcm_tuned)
                               .op("tsamd::rcm_limits", &rcm_limits);
