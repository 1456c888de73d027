// The host steps the samplers (ops_sample.cpp, ops_sample_hetero.cpp, ops_sample_hgt.cpp) are composed of, each held
// ONCE: argument prologue, seed rules, word read-back, planned draw, hop planner, mapped filter, node list, result dicts.
// A new sampler composes these instead of calling the C-ABI for those steps (docs/design/widening.md).  Host-only C++.
#pragma once

#include "ops_common.h"

#include <map>

namespace tsamd_ops {

using node_t = std::string;
using rel_t = std::string;
using edge_t = std::tuple<std::string, std::string, std::string>;
using TensorDict = c10::Dict<std::string, Tensor>;

// ---- argument prologue: the CSR / CSC + ids triple of a homogeneous sampler, checked and made contiguous ------------------
inline void check_graph(const char *op, Tensor &ptr, const char *ptr_name, Tensor &ind, const char *ind_name, Tensor &ids,
                        const char *ids_name) {
  check_index(ptr, ptr_name);
  check_index(ind, ind_name);
  check_index(ids, ids_name);
  TORCH_CHECK(ptr.numel() >= 1, op, ": empty ", ptr_name);
  ptr = ptr.contiguous();
  ind = ind.contiguous();
  ids = ids.contiguous();
}

// ---- the seed of a draw: the rules of the table "Seeds" in docs/design/oracle_parity.md, one function per rule of
// oracle/np_draws.py (host_seed; neighbor_seed = ego_seed = hetero_seed -> draw_seed; redraw_seed); sums wrap mod 2^64 ----
inline uint64_t host_seed() {  // from torch's CPU generator: torch.manual_seed() makes the draws reproducible
  return (uint64_t)torch::randint(0, std::numeric_limits<int64_t>::max(), {1}, torch::TensorOptions().dtype(torch::kLong))
      .item<int64_t>();
}
// n = hop + 1 (neighbor_sample, ego_k_hop_sample_adj) or draw_no (the heterogeneous samplers); sample_adj draws with seed0
inline uint64_t draw_seed(uint64_t seed0, uint64_t n) { return seed0 + 0x9E3779B97F4A7C15ull * n; }
inline uint64_t redraw_seed(uint64_t seed) { return seed ^ 0xA5A5A5A55A5A5A5Aull; }         // tsamd_temporal_redraw
inline uint64_t hgt_select_seed(uint64_t seed0) { return seed0 ^ 0x48475453414D504Cull; }  // "HGTSAMPL": tsamd_hgt_keys / _select

// ---- read-back: the words of some small int64 device tensors, in order, through ONE transfer (THE host sync of the
// samplers; no tensors: no transfer).  What the words mean, and the error a bad-id count raises, is the caller's. ---------
inline std::vector<int64_t> read_words(const std::vector<Tensor> &parts) {
  if (parts.empty()) return {};
  const Tensor host = (parts.size() == 1 ? parts[0] : torch::cat(parts)).cpu();
  return std::vector<int64_t>(host.data_ptr<int64_t>(), host.data_ptr<int64_t>() + host.numel());
}

// ---- the planned draw: one hop over one CSC in two steps, so that a caller can plan SEVERAL draws, read their sizes back
// in ONE transfer and only then allocate and draw (the frontier slices of a hop do not depend on one another) ---------------
struct Drawn {
  Tensor frontier, colptr, row;  // what plan_neighbors was given, in its order
  int64_t k = 0;
  bool replace = false;
  uint64_t seed = 0;
  Tensor out_ptr, info;  // per frontier node: segment pointer; info = (total, #bad ids), on the device
  Tensor nbr, e;         // per draw: the neighbour id and its position in `row`
  int64_t F = 0, T = 0;
  size_t rel = 0;  // plan_hop: the relation's position in the sorted list
};

inline Drawn plan_neighbors(const Tensor &colptr, const Tensor &row, const Tensor &frontier, int64_t k, bool replace,
                            uint64_t seed) {
  const int64_t M = colptr.numel() - 1, F = frontier.numel();
  auto iopt = colptr.options().requires_grad(false);
  Drawn d{frontier, colptr, row, k, replace, seed};
  d.F = F;
  d.out_ptr = torch::empty({F + 1}, iopt);
  d.info = torch::empty({2}, iopt);
  Tensor ws = workspace(tsamd_sample_workspace_bytes(F), colptr);
  check_status(tsamd_sample_plan(colptr.data_ptr<int64_t>(), M, frontier.data_ptr<int64_t>(), F, k, replace ? 1 : 0,
                                 d.out_ptr.data_ptr<int64_t>(), d.info.data_ptr<int64_t>(), ws.data_ptr(),
                                 (size_t)ws.numel(), current_stream(colptr)),
               "tsamd_sample_plan");
  return d;
}

inline void check_plan_ids(const Drawn &d, int64_t bad, const char *noun) {
  TORCH_CHECK_INDEX(bad == 0, "index out of range: ", bad, " ", noun, " ids are outside [0, ", d.colptr.numel() - 1, ")");
}

// ONE host read-back for the sizes of all planned draws; `noun` names the frontier's ids in the error
inline void read_plans(std::vector<Drawn> &plans, const char *noun = "node") {
  std::vector<Tensor> infos;
  for (auto &d : plans) infos.push_back(d.info);
  const std::vector<int64_t> h = read_words(infos);
  for (size_t i = 0; i < plans.size(); ++i) {
    plans[i].T = h[2 * i];
    check_plan_ids(plans[i], h[2 * i + 1], noun);
  }
}

inline void draw_planned(Drawn &d) {
  const int64_t M = d.colptr.numel() - 1;
  auto iopt = d.colptr.options().requires_grad(false);
  void *stream = current_stream(d.colptr);
  d.e = torch::empty({d.T}, iopt);
  d.nbr = torch::empty({d.T}, iopt);
  if (d.T == 0) return;  // nothing to draw (e.g. a relation without entries: its `row` has no storage to pass on)
  if (d.k < 0)
    check_status(tsamd_select_fill(d.colptr.data_ptr<int64_t>(), M, d.row.data_ptr<int64_t>(), d.frontier.data_ptr<int64_t>(),
                                   d.F, d.out_ptr.data_ptr<int64_t>(), d.T, nullptr, d.nbr.data_ptr<int64_t>(),
                                   d.e.data_ptr<int64_t>(), stream),
                 "tsamd_select_fill");
  else
    check_status(tsamd_sample_draw(d.colptr.data_ptr<int64_t>(), d.row.data_ptr<int64_t>(), d.frontier.data_ptr<int64_t>(),
                                   d.F, d.k, d.replace ? 1 : 0, d.seed, d.out_ptr.data_ptr<int64_t>(),
                                   d.e.data_ptr<int64_t>(), d.nbr.data_ptr<int64_t>(), stream),
                 "tsamd_sample_draw");
}

inline Tensor segment_ids(const Tensor &out_ptr, int64_t F, int64_t T) {
  Tensor seg = torch::empty({T}, out_ptr.options());
  check_status(tsamd_ptr2ind(out_ptr.data_ptr<int64_t>(), F, T, seg.data_ptr<int64_t>(), current_stream(out_ptr)),
               "tsamd_ptr2ind");
  return seg;
}

// ---- the hop planner of the heterogeneous samplers: ONE pass over the relations in sorted key order plans the draw of
// every relation that has a frontier.  what(r) -> (the ids to draw for -- none, or undefined: the relation is skipped --,
// k, replace).  draw_no advances for EVERY relation, skipped ones included (np_draws.hetero_seed).  The plans carry their
// relation; the caller reads their sizes (read_plans) or, where an upper bound will do, sets T itself: hgt_sample's
// budget update draws into d.T = d.F * kCap slots without a read-back. ---------------------------------------------------
template <class What>
std::vector<Drawn> plan_hop(const std::vector<rel_t> &rels_sorted, const TensorDict &colptr_dict, const TensorDict &row_dict,
                            uint64_t seed0, uint64_t &draw_no, What what) {
  std::vector<Drawn> plans;
  for (size_t r = 0; r < rels_sorted.size(); ++r) {
    const std::tuple<Tensor, int64_t, bool> w = what(r);
    const Tensor &f = std::get<0>(w);
    ++draw_no;
    if (!f.defined() || f.numel() == 0) continue;
    plans.push_back(plan_neighbors(colptr_dict.at(rels_sorted[r]).contiguous(), row_dict.at(rels_sorted[r]).contiguous(), f,
                                   std::get<1>(w), std::get<2>(w), draw_seed(seed0, draw_no)));
    plans.back().rel = r;
  }
  return plans;
}

// ---- the mapped filter: of T entries, those whose id `nbr` is listed in `assoc` (id -> position, or < 0), in two steps
// like Drawn: count() launches the count and keeps its workspace and device counter (read alone, or batched with other
// words); write(seg, kept) -> (seg of the kept entries, assoc[nbr] of the kept entries, their positions among the T) --------
struct MappedFilter {
  Tensor nbr, assoc, ws, counter;
  static MappedFilter count(const Tensor &nbr, const Tensor &assoc, const Tensor &counter) {
    MappedFilter f{nbr, assoc, workspace(tsamd_filter_tiles_workspace_bytes(nbr.numel()), nbr), counter};
    check_status(tsamd_filter_count(TSAMD_KEEP_COL_MAPPED, nullptr, nbr.data_ptr<int64_t>(), nullptr, assoc.data_ptr<int64_t>(),
                                    nbr.numel(), 0, 0, f.counter.data_ptr<int64_t>(), f.ws.data_ptr(), (size_t)f.ws.numel(),
                                    current_stream(nbr)),
                 "tsamd_filter_count");
    return f;
  }
  std::tuple<Tensor, Tensor, Tensor> write(const Tensor &seg, int64_t kept) const {
    Tensor seg_out = torch::empty({kept}, nbr.options()), map_out = torch::empty_like(seg_out), src = torch::empty_like(seg_out);
    check_status(tsamd_filter_write(TSAMD_KEEP_COL_MAPPED, seg.data_ptr<int64_t>(), nbr.data_ptr<int64_t>(), nullptr,
                                    assoc.data_ptr<int64_t>(), nbr.numel(), 0, 0, ws.data_ptr(), nullptr,
                                    assoc.data_ptr<int64_t>(), 0, 0, seg_out.data_ptr<int64_t>(), map_out.data_ptr<int64_t>(),
                                    src.data_ptr<int64_t>(), current_stream(nbr)),
                 "tsamd_filter_write");
    return std::make_tuple(seg_out, map_out, src);
  }
};

// Entries of the segments `seg_idx` of (ptr, ind) whose index is in `map_idx` (ops_sample.cpp)
std::tuple<Tensor, Tensor, Tensor> induced_entries_bipartite(Tensor seg_idx, Tensor map_idx, int64_t M_map, Tensor ptr,
                                                             Tensor ind, bool first_wins = false);

// ---- The node list of one node type while a multi-hop sampler runs: ids in a capacity buffer, the length in a DEVICE
// counter, and the dense slot[] array of the relabel alive for the whole call (tsamd_relabel_seed / _extend): a hop
// appends without any host read-back; the host learns the lengths once per hop (read_counts), for all types together.
struct NodeList {
  Tensor buf, slot, state;  // state (device) = (length of the list, #bad ids + appends beyond the capacity)
  int64_t n = 0, M = 0;     // n: the length as of the last read-back
  bool seeded = false;

  void init(const Tensor &seeds, int64_t num_nodes) {
    buf = seeds.contiguous();
    n = buf.numel();
    M = num_nodes;
  }
  // the first use as a source type: slot[] is filled and the seeds are entered (legal while count == n)
  void seed() {
    if (seeded) return;
    auto iopt = buf.options().requires_grad(false);
    slot = torch::empty({M}, iopt);
    state = torch::empty({2}, iopt);
    check_status(tsamd_relabel_seed(buf.data_ptr<int64_t>(), n, M, slot.data_ptr<int64_t>(), state.data_ptr<int64_t>(),
                                    state.data_ptr<int64_t>() + 1, /*first_wins=*/1, current_stream(buf)),
                 "tsamd_relabel_seed");
    seeded = true;
  }
  // room for `extra` more ids (called between hops, while count == n)
  void reserve(int64_t extra) {
    if (buf.numel() >= n + extra) return;
    Tensor grown = torch::empty({n + extra}, buf.options());
    if (n > 0) grown.narrow(0, 0, n).copy_(buf.narrow(0, 0, n));
    buf = grown;
  }
  // numbers the ids of nbr (first-occurrence order behind everything listed so far) -> their local ids (or nothing)
  Tensor extend(const Tensor &nbr, bool want_local) {
    const int64_t T = nbr.numel();
    auto iopt = buf.options().requires_grad(false);
    Tensor local = torch::empty({want_local ? T : 0}, iopt);
    if (T == 0) return local;
    Tensor rank = torch::empty({T + 1}, iopt);
    Tensor ws = workspace(tsamd_relabel_workspace_bytes(T), buf);
    check_status(tsamd_relabel_extend(nbr.data_ptr<int64_t>(), T, M, slot.data_ptr<int64_t>(), rank.data_ptr<int64_t>(),
                                      state.data_ptr<int64_t>(), want_local ? local.data_ptr<int64_t>() : nullptr,
                                      buf.data_ptr<int64_t>(), buf.numel(), state.data_ptr<int64_t>() + 1, ws.data_ptr(),
                                      (size_t)ws.numel(), current_stream(buf)),
                 "tsamd_relabel_extend");
    return local;
  }
  // (a view while the buffer is at most twice the list: the copy would cost more than the slack)
  Tensor nodes() const { return buf.numel() == n ? buf : (buf.numel() <= 2 * n ? buf.narrow(0, 0, n) : buf.narrow(0, 0, n).clone()); }
};

// ONE host read-back for the lengths (and error counts) of all lists that were extended
inline void read_counts(std::vector<NodeList *> lists) {
  std::vector<Tensor> words;
  std::vector<NodeList *> live;
  for (NodeList *l : lists)
    if (l->seeded) {
      words.push_back(l->state);
      live.push_back(l);
    }
  const std::vector<int64_t> h = read_words(words);
  for (size_t i = 0; i < live.size(); ++i) {
    TORCH_CHECK_INDEX(h[2 * i + 1] == 0, "node id out of range: ", h[2 * i + 1], " ids are outside [0, ", live[i]->M, ")");
    live[i]->n = h[2 * i];
  }
}

// ---- set-up and packing of the heterogeneous samplers (ops_sample_hetero.cpp) -----------------------------------------------
struct HeteroSetup {
  std::map<rel_t, edge_t> to_edge_type;
  std::map<node_t, int64_t> num_nodes;  // id space of every node type (the dense relabel needs it)
  std::vector<rel_t> rels_sorted;       // the keys of num_neighbors_dict in ascending order (the reference's hop order)
  Tensor any;                           // some device tensor (options / device of the outputs)
};

HeteroSetup hetero_setup(const std::vector<node_t> &node_types, const std::vector<edge_t> &edge_types,
                         const TensorDict &colptr_dict, const TensorDict &row_dict, const TensorDict &input_node_dict,
                         const c10::Dict<rel_t, std::vector<int64_t>> &num_neighbors_dict);

// the four result dicts: a node list per type (omit_empty_types: only of the types that have nodes, as hgt_sample
// returns them), row / col / edge per relation of colptr_dict (empty where nothing was pushed)
inline std::tuple<TensorDict, TensorDict, TensorDict, TensorDict> pack_hetero(
    const std::vector<node_t> &node_types, const TensorDict &colptr_dict, std::map<node_t, Tensor> &samples,
    std::map<rel_t, std::vector<Tensor>> &rows, std::map<rel_t, std::vector<Tensor>> &cols,
    std::map<rel_t, std::vector<Tensor>> &edges, const Tensor &any, bool omit_empty_types = false) {
  auto iopt = any.options().requires_grad(false);
  Tensor none = torch::empty({0}, iopt);
  auto join = [&](std::vector<Tensor> &v) { return v.empty() ? none : (v.size() == 1 ? v[0] : torch::cat(v)); };
  TensorDict out_node, out_row, out_col, out_edge;
  for (const auto &t : node_types) {
    Tensor nodes = samples.count(t) ? samples[t] : none;
    if (!omit_empty_types || nodes.numel() > 0) out_node.insert(t, nodes);
  }
  for (const auto &kv : colptr_dict) {
    out_row.insert(kv.key(), join(rows[kv.key()]));
    out_col.insert(kv.key(), join(cols[kv.key()]));
    out_edge.insert(kv.key(), join(edges[kv.key()]));
  }
  return std::make_tuple(out_node, out_row, out_col, out_edge);
}

}  // namespace tsamd_ops
