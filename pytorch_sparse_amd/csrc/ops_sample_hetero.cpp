// torch operator glue, part 3b: heterogeneous multi-hop sampling (csrc/cpu/neighbor_sample_cpu.cpp:135-507) and the
// set-up it shares with hgt_sample.  See ops_spmm.cpp for the conventions, ops_sample.h for the shared steps.
#include "ops_sample.h"

#include <algorithm>
#include <unordered_map>

namespace tsamd_ops {
namespace {

// largest id of an index array, remembered per (data pointer, length, version counter): see hetero_setup
struct MaxKey {
  const void *data;
  int64_t numel;
  uint64_t version;
  bool operator==(const MaxKey &o) const { return data == o.data && numel == o.numel && version == o.version; }
};
struct MaxKeyHash {
  size_t operator()(const MaxKey &k) const {
    return std::hash<const void *>()(k.data) ^ (std::hash<int64_t>()(k.numel) * 1000003u) ^ (std::hash<uint64_t>()(k.version) * 7919u);
  }
};
// (an entry also holds the tensor's storage WEAKLY: while that storage is alive its address cannot be handed to another
// tensor, so pointer + length + version identify the contents; once it has expired the entry is dead)
struct MaxEntry {
  int64_t value;
  c10::weak_intrusive_ptr<c10::StorageImpl> storage;
};
std::mutex g_max_cache_mutex;
std::unordered_map<MaxKey, MaxEntry, MaxKeyHash> g_max_cache;

bool max_cache_lookup(const MaxKey &k, int64_t *out) {
  std::lock_guard<std::mutex> lock(g_max_cache_mutex);
  auto it = g_max_cache.find(k);
  if (it == g_max_cache.end()) return false;
  if (it->second.storage.expired()) {
    g_max_cache.erase(it);
    return false;
  }
  *out = it->second.value;
  return true;
}
void max_cache_store(const MaxKey &k, int64_t v, const Tensor &t) {
  std::lock_guard<std::mutex> lock(g_max_cache_mutex);
  if (g_max_cache.size() > 1024) g_max_cache.clear();
  g_max_cache.erase(k);
  g_max_cache.emplace(k, MaxEntry{v, c10::weak_intrusive_ptr<c10::StorageImpl>(t.storage().getWeakStorageImpl())});
}

using Slices = std::map<node_t, std::pair<int64_t, int64_t>>;

// what a hop's planner (plan_hop) asks of a relation: the slice of its destination type's ids that the hop draws for
// (none: undefined), and its fan-out in hop ell
Tensor hop_frontier(const Slices &slice, const node_t &dst_t, const Tensor &ids) {
  const int64_t begin = slice.at(dst_t).first, F = slice.at(dst_t).second - begin;
  return F == 0 ? Tensor() : ids.narrow(0, begin, F).contiguous();
}
int64_t fan_out(const c10::Dict<rel_t, std::vector<int64_t>> &num_neighbors_dict, const rel_t &rel, int64_t ell) {
  const auto &fan = num_neighbors_dict.at(rel);
  TORCH_CHECK((int64_t)fan.size() > ell, "num_neighbors_dict[", rel, "] has fewer than num_hops entries");
  return fan[ell];
}

// torch_sparse::hetero_neighbor_sample(str[] node_types, (str, str, str)[] edge_types, Dict(str, Tensor) colptr_dict,
//     Dict(str, Tensor) row_dict, Dict(str, Tensor) input_node_dict, Dict(str, int[]) num_neighbors_dict, int num_hops,
//     bool replace, bool directed) -> (Dict(str, Tensor) node, Dict(str, Tensor) row, Dict(str, Tensor) col, Dict(str, Tensor) edge)
// (reference schema, csrc/neighbor_sample.cpp:29-45; CPU-only there).  Per hop the relations are visited in ascending
// key order; relation src__rel__dst draws in-neighbours (of type src) of the dst nodes discovered in the PREVIOUS hop
// (the slices move at the end of a hop, neighbor_sample_cpu.cpp:216-219, 352-361) and appends the new ones to src's
// node list in first-occurrence order.  Everything that is not random is identical to the reference.
std::tuple<TensorDict, TensorDict, TensorDict, TensorDict> hetero_neighbor_sample(
    const std::vector<node_t> &node_types, const std::vector<edge_t> &edge_types, const TensorDict &colptr_dict,
    const TensorDict &row_dict, const TensorDict &input_node_dict,
    const c10::Dict<rel_t, std::vector<int64_t>> &num_neighbors_dict, int64_t num_hops, bool replace, bool directed) {
  HeteroSetup hs = hetero_setup(node_types, edge_types, colptr_dict, row_dict, input_node_dict, num_neighbors_dict);
  c10::hip::HIPGuard guard(hs.any.get_device());
  auto iopt = hs.any.options().requires_grad(false);
  std::map<node_t, NodeList> lists;
  Slices slice;
  std::vector<NodeList *> all_lists;
  for (const auto &t : node_types) {
    lists[t].init(input_node_dict.contains(t) ? input_node_dict.at(t) : torch::empty({0}, iopt), hs.num_nodes.at(t));
    slice[t] = {0, lists[t].n};
  }
  for (auto &kv : lists) all_lists.push_back(&kv.second);
  std::map<rel_t, std::vector<Tensor>> rows, cols, edges;
  auto dst_of = [&](size_t r) -> const node_t & { return std::get<2>(hs.to_edge_type.at(hs.rels_sorted[r])); };
  const uint64_t seed0 = host_seed();
  uint64_t draw_no = 0;
  // Per hop: every relation's draw is PLANNED first (the frontier slices are fixed for the hop), ONE transfer reads all
  // their sizes; the draws and relabels of the hop then run back to back on the device (NodeList); a second transfer at
  // the end of the hop reads the new length of every node list.  Two host read-backs per hop whatever the number of
  // relations (round 5: two per relation and hop).
  for (int64_t ell = 0; ell < num_hops; ++ell) {
    std::vector<Drawn> plans = plan_hop(
        hs.rels_sorted, colptr_dict, row_dict, seed0, draw_no, [&](size_t r) {
          const int64_t k = fan_out(num_neighbors_dict, hs.rels_sorted[r], ell);
          return std::make_tuple(hop_frontier(slice, dst_of(r), lists.at(dst_of(r)).buf), k, replace);
        });
    read_plans(plans);  // host sync 1 of the hop
    std::map<node_t, int64_t> extra;
    for (const Drawn &d : plans) extra[std::get<0>(hs.to_edge_type.at(hs.rels_sorted[d.rel]))] += d.T;
    for (const auto &kv : extra) {
      lists.at(kv.first).seed();
      lists.at(kv.first).reserve(kv.second);
    }
    for (Drawn &d : plans) {
      const rel_t &rel = hs.rels_sorted[d.rel];
      const edge_t &et = hs.to_edge_type.at(rel);
      const int64_t begin = slice.at(std::get<2>(et)).first;
      draw_planned(d);
      Tensor local = lists.at(std::get<0>(et)).extend(d.nbr, directed);
      if (directed) {
        Tensor seg = segment_ids(d.out_ptr, d.F, d.T);
        rows[rel].push_back(local);
        cols[rel].push_back(begin > 0 ? seg + begin : seg);
        edges[rel].push_back(d.e);
      }
    }
    if (!plans.empty()) read_counts(all_lists);  // host sync 2 of the hop
    for (const auto &t : node_types) slice[t] = {slice[t].second, lists[t].n};
  }
  std::map<node_t, Tensor> samples;
  for (const auto &t : node_types) samples[t] = lists[t].nodes();
  if (!directed) {  // every stored edge between the sampled nodes, relation by relation (neighbor_sample_cpu.cpp:366-397)
    for (const auto &kv : colptr_dict) {
      const edge_t &et = hs.to_edge_type.at(kv.key());
      const node_t &src_t = std::get<0>(et), &dst_t = std::get<2>(et);
      if (samples.at(dst_t).numel() == 0 || samples.at(src_t).numel() == 0) continue;
      auto sub = induced_entries_bipartite(samples.at(dst_t), samples.at(src_t), hs.num_nodes.at(src_t),
                                           kv.value().contiguous(), row_dict.at(kv.key()).contiguous(), /*first_wins=*/true);
      rows[kv.key()].push_back(std::get<1>(sub));
      cols[kv.key()].push_back(std::get<0>(sub));
      edges[kv.key()].push_back(std::get<2>(sub));
    }
  }
  return pack_hetero(node_types, colptr_dict, samples, rows, cols, edges, hs.any);
}

// torch_sparse::hetero_temporal_neighbor_sample(..., Dict(str, Tensor) node_time_dict, int num_hops, bool replace,
//     bool directed)                               (reference schema, csrc/neighbor_sample.cpp:47-63; directed only)
// The hetero sampler with a time constraint: a neighbour v of type src may be drawn for a node of root time t only if
// node_time[src][v] <= t (types without a time tensor are unconstrained), every root keeps its own computation tree --
// nodes are (node, root) pairs -- and a drawn node inherits the root time of the node it was drawn for.
//   take-all / without replacement: the draw of the untimed sampler, then the violating draws are dropped (as in
//       neighbor_sample_cpu.cpp:240-262, 305-330: fewer than num_neighbors may remain);
//   with replacement: num_neighbors uniform draws among the neighbours that satisfy the constraint (the reference
//       redraws until one does, :268-300 -- and never returns when none does; here such a node draws nothing).
// Device-driven inside a (relation, hop) (csrc/sample.hip, tsamd_temporal_*): the constraint is a FLAG per draw, the
// (node, root) pairs are numbered by one stable sort of old pairs + candidates, and only then ONE transfer reads
// (#draws kept, #new pairs) and one kernel writes the compacted outputs.  Host read-backs: one per hop (the sizes of all
// the hop's draws) + one per relation and hop.  (Round 5: an ATen composition with four to five per relation and hop.)
std::tuple<TensorDict, TensorDict, TensorDict, TensorDict> hetero_temporal_neighbor_sample(
    const std::vector<node_t> &node_types, const std::vector<edge_t> &edge_types, const TensorDict &colptr_dict,
    const TensorDict &row_dict, const TensorDict &input_node_dict,
    const c10::Dict<rel_t, std::vector<int64_t>> &num_neighbors_dict, const TensorDict &node_time_dict, int64_t num_hops,
    bool replace, bool directed) {
  TORCH_CHECK(directed, "Temporal sampling requires 'directed' sampling");
  HeteroSetup hs = hetero_setup(node_types, edge_types, colptr_dict, row_dict, input_node_dict, num_neighbors_dict);
  c10::hip::HIPGuard guard(hs.any.get_device());
  auto iopt = hs.any.options().requires_grad(false);
  std::map<node_t, Tensor> tnode, troot, ttime;
  Slices slice;
  int64_t R = 1;  // number of roots
  for (const auto &kv : input_node_dict) R = std::max<int64_t>(R, kv.value().numel());
  for (const auto &t : node_types) {
    if (input_node_dict.contains(t)) {
      TORCH_CHECK(node_time_dict.contains(t), "hetero_temporal_neighbor_sample: no node_time for input type ", t);
      Tensor x = input_node_dict.at(t).contiguous();
      check_index(node_time_dict.at(t), "node_time");
      tnode[t] = x;
      troot[t] = torch::arange(x.numel(), iopt);
      ttime[t] = node_time_dict.at(t).index_select(0, x);
    } else {
      tnode[t] = torch::empty({0}, iopt);
      troot[t] = torch::empty({0}, iopt);
      ttime[t] = torch::empty({0}, iopt);
    }
    slice[t] = {0, tnode[t].numel()};
  }
  std::map<rel_t, std::vector<Tensor>> rows, cols, edges;
  auto dst_of = [&](size_t r) -> const node_t & { return std::get<2>(hs.to_edge_type.at(hs.rels_sorted[r])); };
  const uint64_t seed0 = host_seed();
  uint64_t draw_no = 0;
  for (int64_t ell = 0; ell < num_hops; ++ell) {
    std::vector<Drawn> plans = plan_hop(
        hs.rels_sorted, colptr_dict, row_dict, seed0, draw_no, [&](size_t r) {
          const int64_t k = fan_out(num_neighbors_dict, hs.rels_sorted[r], ell);
          // draws with replacement are made among the VALID neighbours: list them all
          return std::make_tuple(hop_frontier(slice, dst_of(r), tnode.at(dst_of(r))), replace && k >= 0 ? (int64_t)-1 : k, false);
        });
    read_plans(plans);  // the hop's one read-back of draw sizes
    for (Drawn &d : plans) {
      const rel_t &rel = hs.rels_sorted[d.rel];
      const edge_t &et = hs.to_edge_type.at(rel);
      const node_t &src_t = std::get<0>(et), &dst_t = std::get<2>(et);
      const int64_t k = num_neighbors_dict.at(rel)[ell];
      const int64_t begin = slice.at(dst_t).first, F = d.F;
      const bool redraw = replace && k >= 0;
      if (d.T == 0) continue;
      draw_planned(d);
      void *stream = current_stream(d.colptr);
      Tensor f_root = troot.at(dst_t).narrow(0, begin, F).contiguous(), f_time = ttime.at(dst_t).narrow(0, begin, F).contiguous();
      Tensor src_time;
      if (node_time_dict.contains(src_t)) {
        src_time = node_time_dict.at(src_t).contiguous();
        check_index(src_time, "node_time");
      }
      int64_t T = d.T;
      Tensor seg = segment_ids(d.out_ptr, F, T), nbr = d.nbr, e = d.e;
      Tensor keep = torch::empty({T}, iopt);
      check_status(tsamd_temporal_mark(nbr.data_ptr<int64_t>(), seg.data_ptr<int64_t>(), T,
                                       src_time.defined() ? src_time.data_ptr<int64_t>() : nullptr,
                                       f_time.data_ptr<int64_t>(), keep.data_ptr<int64_t>(), stream),
                   "tsamd_temporal_mark");
      if (redraw) {
        if (k == 0) continue;
        const int64_t T2 = F * k;
        Tensor nbr2 = torch::empty({T2}, iopt), e2 = torch::empty({T2}, iopt), seg2 = torch::empty({T2}, iopt),
               keep2 = torch::empty({T2}, iopt);
        Tensor ws = workspace(tsamd_temporal_redraw_workspace_bytes(T), nbr);
        check_status(tsamd_temporal_redraw(d.out_ptr.data_ptr<int64_t>(), F, T, k, redraw_seed(d.seed),
                                           nbr.data_ptr<int64_t>(), e.data_ptr<int64_t>(), keep.data_ptr<int64_t>(),
                                           nbr2.data_ptr<int64_t>(), e2.data_ptr<int64_t>(), seg2.data_ptr<int64_t>(),
                                           keep2.data_ptr<int64_t>(), ws.data_ptr(), (size_t)ws.numel(), stream),
                     "tsamd_temporal_redraw");
        nbr = nbr2;
        e = e2;
        seg = seg2;
        keep = keep2;
        T = T2;
      }
      const int64_t n_old = tnode.at(src_t).numel();
      Tensor local = torch::empty({T}, iopt), keep_rank = torch::empty({T + 1}, iopt), open_rank = torch::empty({T + 1}, iopt);
      Tensor info = torch::empty({2}, iopt);
      Tensor ws = workspace(tsamd_temporal_relabel_workspace_bytes(n_old, T), nbr);
      check_status(tsamd_temporal_relabel(tnode.at(src_t).data_ptr<int64_t>(), troot.at(src_t).data_ptr<int64_t>(), n_old,
                                          nbr.data_ptr<int64_t>(), seg.data_ptr<int64_t>(), f_root.data_ptr<int64_t>(),
                                          keep.data_ptr<int64_t>(), T, hs.num_nodes.at(src_t), R,
                                          local.data_ptr<int64_t>(), keep_rank.data_ptr<int64_t>(),
                                          open_rank.data_ptr<int64_t>(), info.data_ptr<int64_t>(), ws.data_ptr(),
                                          (size_t)ws.numel(), stream),
                   "tsamd_temporal_relabel");
      const std::vector<int64_t> host = read_words({info});  // the relation's one read-back
      const int64_t n_keep = host[0], n_open = host[1];
      if (n_keep == 0) continue;
      Tensor r_out = torch::empty({n_keep}, iopt), c_out = torch::empty({n_keep}, iopt), e_out = torch::empty({n_keep}, iopt);
      Tensor node_new = tnode.at(src_t), root_new = troot.at(src_t), time_new = ttime.at(src_t);
      auto grown = [&](const Tensor &old) {  // room for the new pairs behind the old ones
        Tensor g = torch::empty({n_old + n_open}, iopt);
        if (n_old > 0) g.narrow(0, 0, n_old).copy_(old);
        return g;
      };
      if (n_open > 0) node_new = grown(node_new), root_new = grown(root_new), time_new = grown(time_new);
      check_status(tsamd_temporal_emit(nbr.data_ptr<int64_t>(), e.data_ptr<int64_t>(), seg.data_ptr<int64_t>(),
                                       f_root.data_ptr<int64_t>(), f_time.data_ptr<int64_t>(), keep_rank.data_ptr<int64_t>(),
                                       open_rank.data_ptr<int64_t>(), local.data_ptr<int64_t>(), T, begin,
                                       r_out.data_ptr<int64_t>(), c_out.data_ptr<int64_t>(), e_out.data_ptr<int64_t>(),
                                       node_new.data_ptr<int64_t>() + n_old, root_new.data_ptr<int64_t>() + n_old,
                                       time_new.data_ptr<int64_t>() + n_old, stream),
                   "tsamd_temporal_emit");
      rows[rel].push_back(r_out);
      cols[rel].push_back(c_out);
      edges[rel].push_back(e_out);
      tnode[src_t] = node_new;
      troot[src_t] = root_new;
      ttime[src_t] = time_new;
    }
    for (const auto &t : node_types) slice[t] = {slice[t].second, tnode[t].numel()};
  }
  return pack_hetero(node_types, colptr_dict, tnode, rows, cols, edges, hs.any);
}

}  // namespace

HeteroSetup hetero_setup(const std::vector<node_t> &node_types, const std::vector<edge_t> &edge_types,
                         const TensorDict &colptr_dict, const TensorDict &row_dict, const TensorDict &input_node_dict,
                         const c10::Dict<rel_t, std::vector<int64_t>> &num_neighbors_dict) {
  HeteroSetup hs;
  for (const auto &k : edge_types) hs.to_edge_type[std::get<0>(k) + "__" + std::get<1>(k) + "__" + std::get<2>(k)] = k;
  for (const auto &t : node_types) hs.num_nodes[t] = 0;
  bool have = false;
  for (const auto &kv : colptr_dict) {
    const Tensor &cp = kv.value();
    check_index(cp, "colptr");
    TORCH_CHECK(cp.numel() >= 1, "hetero_neighbor_sample: empty colptr");
    TORCH_CHECK(hs.to_edge_type.count(kv.key()), "unknown relation ", kv.key());
    if (!have) {
      hs.any = cp;
      have = true;
    }
    auto &n = hs.num_nodes[std::get<2>(hs.to_edge_type.at(kv.key()))];  // destination type: one column per node
    n = std::max<int64_t>(n, cp.numel() - 1);
  }
  TORCH_CHECK(have, "hetero_neighbor_sample: no relations");
  // source types: the largest id any relation or input refers to.  The relations' row arrays are the graph -- the same
  // tensors call after call: their maxima are remembered per (data pointer, length, version counter); what is left
  // (first call: every array; later: the input nodes of the mini-batch) is reduced on the device and read back in ONE
  // transfer (round 5 paid one reduction over the relation's whole edge list + one host sync per dict entry, per call).
  std::vector<Tensor> pending;              // 0-dim device maxima still to be read
  std::vector<int64_t *> pending_dst;       // where each goes (num_nodes entry), as max(n, value + 1)
  std::vector<MaxKey> pending_key;          // cache slot to fill (data == nullptr: not cached)
  std::vector<Tensor> pending_src;
  for (const auto &kv : row_dict) {
    const Tensor &r = kv.value();
    check_index(r, "row");
    auto &n = hs.num_nodes[std::get<0>(hs.to_edge_type.at(kv.key()))];
    if (r.numel() == 0) continue;
    const MaxKey key{r.data_ptr(), r.numel(), (uint64_t)r._version()};
    int64_t cached = 0;
    if (max_cache_lookup(key, &cached)) {
      n = std::max<int64_t>(n, cached + 1);
    } else {
      pending.push_back(r.max());
      pending_dst.push_back(&n);
      pending_key.push_back(key);
      pending_src.push_back(r);
    }
  }
  for (const auto &kv : input_node_dict) {
    const Tensor &x = kv.value();
    check_index(x, "input_node");
    TORCH_CHECK(hs.num_nodes.count(kv.key()), "unknown node type ", kv.key());
    if (x.numel() == 0) continue;
    pending.push_back(x.max());
    pending_dst.push_back(&hs.num_nodes[kv.key()]);
    pending_key.push_back(MaxKey{nullptr, 0, 0});
    pending_src.push_back(x);
  }
  if (!pending.empty()) {
    const Tensor host = torch::stack(pending).cpu();  // the one read-back of the set-up
    const int64_t *h = host.data_ptr<int64_t>();
    for (size_t i = 0; i < pending.size(); ++i) {
      *pending_dst[i] = std::max<int64_t>(*pending_dst[i], h[i] + 1);
      if (pending_key[i].data != nullptr) max_cache_store(pending_key[i], h[i], pending_src[i]);
    }
  }
  for (const auto &kv : num_neighbors_dict) hs.rels_sorted.push_back(kv.key());
  std::sort(hs.rels_sorted.begin(), hs.rels_sorted.end());
  return hs;
}

}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_sample_hetero =
    torch::RegisterOperators()
        .op("torch_sparse::hetero_neighbor_sample", &hetero_neighbor_sample)
        .op("torch_sparse::hetero_temporal_neighbor_sample", &hetero_temporal_neighbor_sample);
