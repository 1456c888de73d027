// torch operator glue, part 3: the mini-batch producers: random walks, neighbour
// sampling, relabelling, induced sub-graphs, ego sub-graphs.  See ops_spmm.cpp for the conventions and ops_sample.h for
// the steps the samplers share; the heterogeneous samplers are ops_sample_hetero.cpp, hgt_sample is ops_sample_hgt.cpp.
#include "ops_sample.h"

#include <algorithm>

namespace tsamd_ops {
namespace {

// ---- mini-batch producers (include/tsamd.h) -----------------------------
// walk with the uniform floats handed in: out[n, L+1] is a pure function of the inputs
Tensor random_walk_with_rand(Tensor rowptr, Tensor col, Tensor start, Tensor rand) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  check_index(start, "start");
  check_gpu(rand, "rand");
  TORCH_CHECK(rand.dim() == 2 && rand.size(0) == start.numel() && rand.scalar_type() == at::kFloat,
              "rand must be float32 [start.numel(), walk_length]");
  c10::hip::HIPGuard guard(rowptr.get_device());
  rowptr = rowptr.contiguous();
  col = col.contiguous();
  start = start.contiguous();
  rand = rand.contiguous();
  const int64_t n = start.numel(), L = rand.size(1);
  Tensor out = torch::empty({n, L + 1}, start.options());
  check_status(tsamd_random_walk(rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                                 start.data_ptr<int64_t>(), rand.data_ptr<float>(), n, L,
                                 out.data_ptr<int64_t>(), current_stream(rowptr)),
               "tsamd_random_walk");
  return out;
}

// torch_sparse::random_walk(Tensor rowptr, Tensor col, Tensor start, int walk_length) -> Tensor
// (reference schema, csrc/rw.cpp:21-36); the floats come from torch's generator of the device.
Tensor random_walk(Tensor rowptr, Tensor col, Tensor start, int64_t walk_length) {
  check_index(start, "start");
  TORCH_CHECK(walk_length >= 0, "walk_length must be non-negative");
  Tensor rand = torch::rand({start.numel(), walk_length}, start.options().dtype(torch::kFloat));
  return random_walk_with_rand(rowptr, col, start, rand);
}

struct Relabelled {
  Tensor local, n_id;
  int64_t n_new;
};

// first-occurrence relabel of nbr against the seeds idx over M node ids (one host sync)
Relabelled relabel_impl(const Tensor &idx, const Tensor &nbr, int64_t M, bool want_local) {
  const int64_t n = idx.numel(), T = nbr.numel();
  auto iopt = idx.options().requires_grad(false);
  void *stream = current_stream(idx);
  Tensor slot = torch::empty({M}, iopt), rank = torch::empty({T + 1}, iopt);
  Tensor info = torch::empty({2}, iopt);
  Tensor ws = workspace(tsamd_relabel_workspace_bytes(T), idx);
  check_status(tsamd_relabel_plan(idx.data_ptr<int64_t>(), n, nbr.data_ptr<int64_t>(), T, M,
                                  slot.data_ptr<int64_t>(), rank.data_ptr<int64_t>(),
                                  info.data_ptr<int64_t>(), ws.data_ptr(), (size_t)ws.numel(), stream),
               "tsamd_relabel_plan");
  const std::vector<int64_t> h = read_words({info});  // (#new nodes, #bad ids)
  TORCH_CHECK_INDEX(h[1] == 0, "node id out of range: ", h[1], " ids are outside [0, ", M, ")");
  Relabelled r{torch::empty({want_local ? T : 0}, iopt), torch::empty({n + h[0]}, iopt), h[0]};
  check_status(tsamd_relabel_apply(idx.data_ptr<int64_t>(), n, nbr.data_ptr<int64_t>(), T, M,
                                   slot.data_ptr<int64_t>(), rank.data_ptr<int64_t>(),
                                   want_local ? r.local.data_ptr<int64_t>() : nullptr,
                                   r.n_id.data_ptr<int64_t>(), stream),
               "tsamd_relabel_apply");
  return r;
}

// torch_sparse::sample_adj(Tensor rowptr, Tensor col, Tensor idx, int num_neighbors, bool replace)
//   -> (Tensor rowptr, Tensor col, Tensor n_id, Tensor e_id)      (reference schema, csrc/sample.cpp)
// Adjacency of the seeds idx restricted to sampled neighbours, columns renumbered: seeds first, new
// nodes in first-occurrence order; every row sorted by the new column id.  Two host syncs.
std::tuple<Tensor, Tensor, Tensor, Tensor> sample_adj(Tensor rowptr, Tensor col, Tensor idx,
                                                      int64_t num_neighbors, bool replace) {
  check_graph("sample_adj", rowptr, "rowptr", col, "col", idx, "idx");
  c10::hip::HIPGuard guard(rowptr.get_device());
  const int64_t M = rowptr.numel() - 1, n = idx.numel();
  auto iopt = rowptr.options().requires_grad(false);
  void *stream = current_stream(rowptr);
  std::vector<Drawn> plan{plan_neighbors(rowptr, col, idx, num_neighbors, replace, 0)};
  read_plans(plan, "seed");  // sync 1
  Drawn &d = plan[0];
  // the draw's seed is seed0 itself; taking every neighbour leaves torch's CPU generator untouched
  if (num_neighbors >= 0) d.seed = host_seed();
  draw_planned(d);
  Relabelled r = relabel_impl(idx, d.nbr, M, true);  // sync 2
  // rows sorted by the new column id (sample_cpu.cpp:124-129)
  Tensor row = segment_ids(d.out_ptr, n, d.T);
  const int64_t Nloc = n + r.n_new;
  Tensor col_s = torch::empty({d.T}, iopt), perm = torch::empty({d.T}, iopt);
  Tensor ws2 = workspace(tsamd_sort_coo_workspace_bytes(d.T), rowptr);
  check_status(tsamd_sort_coo(row.data_ptr<int64_t>(), r.local.data_ptr<int64_t>(), d.T, n > 0 ? n : 1,
                              Nloc > 0 ? Nloc : 1, nullptr, col_s.data_ptr<int64_t>(),
                              perm.data_ptr<int64_t>(), ws2.data_ptr(), (size_t)ws2.numel(), stream),
               "tsamd_sort_coo");
  return std::make_tuple(d.out_ptr, col_s, r.n_id, d.e.index_select(0, perm));
}

// torch_sparse::relabel(Tensor col, Tensor idx) -> (Tensor col, Tensor idx)  (csrc/relabel.cpp:18-29)
std::tuple<Tensor, Tensor> relabel(Tensor col, Tensor idx) {
  check_index(col, "col");
  check_index(idx, "idx");
  c10::hip::HIPGuard guard(col.get_device());
  col = col.contiguous();
  idx = idx.contiguous();
  // the reference keys a hash map, here the id space must be known: one extra sync for the max id
  int64_t M = 0;
  if (col.numel() > 0) M = std::max(M, col.max().item<int64_t>() + 1);
  if (idx.numel() > 0) M = std::max(M, idx.max().item<int64_t>() + 1);
  Relabelled r = relabel_impl(idx, col, M, true);
  return std::make_tuple(r.local, r.n_id);
}

// torch_sparse::relabel_one_hop(Tensor rowptr, Tensor col, Tensor? value, Tensor idx, bool bipartite)
//   -> (Tensor rowptr, Tensor col, Tensor? value, Tensor idx)           (csrc/relabel.cpp:32-45)
std::tuple<Tensor, Tensor, OptTensor, Tensor> relabel_one_hop(Tensor rowptr, Tensor col,
                                                              OptTensor value, Tensor idx,
                                                              bool bipartite) {
  check_graph("relabel_one_hop", rowptr, "rowptr", col, "col", idx, "idx");
  c10::hip::HIPGuard guard(rowptr.get_device());
  auto sel = select_segments(rowptr, col, idx, false, true);  // (out_ptr, -, nbr, pos), sync 1
  Tensor out_ptr = std::get<0>(sel), nbr = std::get<2>(sel), pos = std::get<3>(sel);
  Relabelled r = relabel_impl(idx, nbr, rowptr.numel() - 1, true);  // sync 2
  OptTensor out_value = std::nullopt;
  if (value.has_value()) out_value = value.value().index_select(0, pos);
  if (!bipartite)
    out_ptr = torch::cat({out_ptr, torch::full({r.n_new}, nbr.numel(), out_ptr.options())});
  return std::make_tuple(out_ptr, r.local, out_value, r.n_id);
}

// torch_sparse::saint_subgraph(Tensor idx, Tensor rowptr, Tensor row, Tensor col)
//   -> (Tensor row, Tensor col, Tensor edge_index)                       (csrc/saint.cpp:20-33)
// Sub-graph induced by the node subset idx, nodes renumbered by their position in idx; rows in
// idx order, every row keeps its stored column order (as subgraph_cpu does).
std::tuple<Tensor, Tensor, Tensor> saint_subgraph(Tensor idx, Tensor rowptr, Tensor row, Tensor col) {
  check_graph("saint_subgraph", rowptr, "rowptr", col, "col", idx, "idx");
  c10::hip::HIPGuard guard(rowptr.get_device());
  return induced_entries_bipartite(idx, idx, rowptr.numel() - 1, rowptr, col);
}

// torch_sparse::neighbor_sample(Tensor colptr, Tensor row, Tensor input_node, int[] num_neighbors,
//                               bool replace, bool directed) -> (Tensor node, Tensor row, Tensor col, Tensor edge)
// (reference schema, csrc/neighbor_sample.cpp:18-27; CPU-only there).  Multi-hop sampling on the
// CSC view: hop l draws num_neighbors[l] in-neighbours of every node discovered in hop l-1; nodes
// are numbered in first-occurrence order across hops; an edge is (local id of the drawn source,
// local id of the frontier node, position in `row`).  directed=false returns instead every stored
// edge between the sampled nodes.  Two host read-backs per hop (size of the draw; length of the node list); the
// relabel's slot array is set up once per call (round 6; before: an M x 8-byte fill and a re-seeding of every node
// sampled so far in every hop).
std::tuple<Tensor, Tensor, Tensor, Tensor> neighbor_sample(Tensor colptr, Tensor row, Tensor input_node,
                                                           std::vector<int64_t> num_neighbors, bool replace, bool directed) {
  check_graph("neighbor_sample", colptr, "colptr", row, "row", input_node, "input_node");
  c10::hip::HIPGuard guard(colptr.get_device());
  auto iopt = colptr.options().requires_grad(false);
  NodeList list;
  list.init(input_node, colptr.numel() - 1);
  int64_t begin = 0, end = list.n;
  std::vector<Tensor> rows, cols, edges;
  const uint64_t seed0 = host_seed();
  for (size_t ell = 0; ell < num_neighbors.size(); ++ell) {
    const int64_t F = end - begin;
    std::vector<Drawn> plan{plan_neighbors(colptr, row, list.buf.narrow(0, begin, F), num_neighbors[ell], replace,
                                           draw_seed(seed0, ell + 1))};
    read_plans(plan);  // sync 1
    Drawn &d = plan[0];
    list.seed();
    list.reserve(d.T);
    draw_planned(d);
    Tensor local = list.extend(d.nbr, directed);
    if (directed) {
      Tensor seg = segment_ids(d.out_ptr, F, d.T);
      rows.push_back(local);
      cols.push_back(begin > 0 ? seg + begin : seg);
      edges.push_back(d.e);
    }
    read_counts({&list});  // sync 2
    begin = end;
    end = list.n;
  }
  Tensor samples = list.nodes();
  if (!directed) {
    auto sub = induced_entries_bipartite(samples, samples, colptr.numel() - 1, colptr, row, /*first_wins=*/true);
    return std::make_tuple(samples, std::get<1>(sub), std::get<0>(sub), std::get<2>(sub));
  }
  Tensor none = torch::empty({0}, iopt);
  return std::make_tuple(samples, rows.empty() ? none : torch::cat(rows), cols.empty() ? none : torch::cat(cols),
                         edges.empty() ? none : torch::cat(edges));
}

// torch_sparse::ego_k_hop_sample_adj(Tensor rowptr, Tensor col, Tensor idx, int depth, int num_neighbors, bool replace)
//   -> (Tensor rowptr, Tensor col, Tensor n_id, Tensor e_id, Tensor ptr, Tensor root_n_id)
// (reference schema, csrc/ego_sample.cpp; CPU-only there, csrc/cpu/ego_sample_cpu.cpp).  Every seed g grows its own
// depth-hop node set S_g (every draw of a hop is expanded in the next one, duplicates included); n_id lists each S_g in
// ascending id order, and the sub-graph induced by S_g follows in (row ascending, stored order) -- the reference's
// outputs bit for bit once the sets are fixed.  Host read-backs: one per hop (the number of draws) + the number of
// distinct (seed, node) pairs + the number of candidate entries V + the number of kept entries; none per seed or row.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> ego_k_hop_sample_adj(Tensor rowptr, Tensor col, Tensor idx,
                                                                                int64_t depth, int64_t num_neighbors,
                                                                                bool replace) {
  check_graph("ego_k_hop_sample_adj", rowptr, "rowptr", col, "col", idx, "idx");
  c10::hip::HIPGuard guard(rowptr.get_device());
  const int64_t M = rowptr.numel() - 1, n = idx.numel();
  auto iopt = rowptr.options().requires_grad(false);
  if (n == 0) {  // (the reference's loops have nothing to do and torch::cat gets an empty list)
    auto none = [&]() { return torch::empty({0}, iopt); };
    return std::make_tuple(torch::zeros({1}, iopt), none(), none(), none(), torch::zeros({1}, iopt), none());
  }
  TORCH_CHECK_INDEX(M > 0, "index out of range: the graph has no nodes");
  void *stream = current_stream(rowptr);
  // device words: [0, 4) the coalesce's counts, [4] #ids outside [0, M) (all steps add to it), [5] draws of the hop,
  // [6, 8) select_plan's info (V, #bad ids) -- [7] then receives the number of kept entries
  Tensor words = torch::zeros({8}, iopt);
  int64_t *w = words.data_ptr<int64_t>();
  auto check_ids = [&](int64_t bad) {
    TORCH_CHECK_INDEX(bad == 0, "index out of range: ", bad, " node ids are outside [0, ", M, ")");
  };

  Tensor seg0 = torch::empty({n}, iopt), node0 = torch::empty({n}, iopt);
  check_status(tsamd_ego_seeds(idx.data_ptr<int64_t>(), n, M, seg0.data_ptr<int64_t>(), node0.data_ptr<int64_t>(), w + 4,
                               stream),
               "tsamd_ego_seeds");
  std::vector<Tensor> segs{seg0}, nodes{node0};
  Tensor frontier = node0, fseg = seg0;
  const uint64_t seed0 = host_seed();
  for (int64_t hop = 0; hop < depth && num_neighbors > 0; ++hop) {  // k <= 0 draws nothing (ego_sample_cpu.cpp:49-73)
    const int64_t F = frontier.numel();
    if (F == 0) break;
    Tensor out_ptr = torch::empty({F + 1}, iopt);
    Tensor ws = workspace(tsamd_ego_plan_workspace_bytes(F), rowptr);
    check_status(tsamd_ego_plan(rowptr.data_ptr<int64_t>(), M, frontier.data_ptr<int64_t>(), F, num_neighbors,
                                out_ptr.data_ptr<int64_t>(), w + 5, w + 4, ws.data_ptr(), (size_t)ws.numel(), stream),
                 "tsamd_ego_plan");
    const std::vector<int64_t> h = read_words({words.narrow(0, 4, 2)});  // read-back: the hop's number of draws
    check_ids(h[0]);
    const int64_t T = h[1];
    Tensor nbr = torch::empty({T}, iopt), sg = torch::empty({T}, iopt);
    check_status(tsamd_ego_draw(rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), M, frontier.data_ptr<int64_t>(),
                                fseg.data_ptr<int64_t>(), F, num_neighbors, replace ? 1 : 0,
                                draw_seed(seed0, hop + 1), out_ptr.data_ptr<int64_t>(), T,
                                nbr.data_ptr<int64_t>(), sg.data_ptr<int64_t>(), w + 4, stream),
                 "tsamd_ego_draw");
    segs.push_back(sg);
    nodes.push_back(nbr);
    frontier = nbr;
    fseg = sg;
  }

  // the node sets: distinct (seed, node) pairs in row-major order
  Tensor seg = segs.size() == 1 ? segs[0] : torch::cat(segs), node = nodes.size() == 1 ? nodes[0] : torch::cat(nodes);
  const int64_t L = seg.numel();
  Tensor row_t = torch::empty({L}, iopt), col_t = torch::empty({L}, iopt);
  Tensor row_u = torch::empty({L}, iopt), col_u = torch::empty({L}, iopt), seg_ptr = torch::empty({L + 1}, iopt);
  {
    Tensor ws = workspace(tsamd_sort_coalesce_workspace_bytes(L), rowptr);
    check_status(tsamd_sort_coalesce_reduce(seg.data_ptr<int64_t>(), node.data_ptr<int64_t>(), L, n, M,
                                            row_t.data_ptr<int64_t>(), col_t.data_ptr<int64_t>(),
                                            row_u.data_ptr<int64_t>(), col_u.data_ptr<int64_t>(),
                                            seg_ptr.data_ptr<int64_t>(), w, TSAMD_F32, TSAMD_SUM, nullptr, nullptr,
                                            nullptr, ws.data_ptr(), (size_t)ws.numel(), stream),
                 "tsamd_sort_coalesce_reduce");
  }
  const std::vector<int64_t> hd = read_words({words.narrow(0, 2, 3)});  // read-back: the number of distinct pairs
  check_ids(hd[2]);
  const int64_t D = hd[0];
  Tensor n_id = D == L ? col_u : col_u.narrow(0, 0, D).clone();
  Tensor n_seg = row_u.narrow(0, 0, D);
  Tensor ptr = torch::empty({n + 1}, iopt), root_n_id = torch::empty({n}, iopt);
  check_status(tsamd_ind2ptr(n_seg.data_ptr<int64_t>(), n, D, ptr.data_ptr<int64_t>(), stream), "tsamd_ind2ptr");
  check_status(tsamd_ego_roots(idx.data_ptr<int64_t>(), n, ptr.data_ptr<int64_t>(), n_id.data_ptr<int64_t>(),
                               root_n_id.data_ptr<int64_t>(), stream),
               "tsamd_ego_roots");

  // the induced sub-graphs: every stored entry of every row of n_id is a candidate
  Tensor vptr = torch::empty({D + 1}, iopt);
  {
    Tensor ws = workspace(tsamd_select_workspace_bytes(D), rowptr);
    check_status(tsamd_select_plan(rowptr.data_ptr<int64_t>(), M, n_id.data_ptr<int64_t>(), D,
                                   vptr.data_ptr<int64_t>(), w + 6, ws.data_ptr(), (size_t)ws.numel(), stream),
                 "tsamd_select_plan");
  }
  const int64_t V = read_words({words.narrow(0, 6, 1)})[0];  // read-back: the number of candidates
  Tensor ws = workspace(tsamd_ego_induced_workspace_bytes(V), rowptr);
  check_status(tsamd_ego_induced_count(rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), M, n_id.data_ptr<int64_t>(),
                                       n_seg.data_ptr<int64_t>(), D, ptr.data_ptr<int64_t>(), vptr.data_ptr<int64_t>(), V,
                                       w + 7, w + 4, ws.data_ptr(), (size_t)ws.numel(), stream),
               "tsamd_ego_induced_count");
  const std::vector<int64_t> hk = read_words({words.narrow(0, 4, 4)});  // read-back: the number of kept entries
  check_ids(hk[0]);
  const int64_t K = hk[3];
  Tensor row_o = torch::empty({K}, iopt), col_o = torch::empty({K}, iopt), e_id = torch::empty({K}, iopt);
  if (K > 0)  // (empty outputs have no storage to pass on)
    check_status(tsamd_ego_induced_write(rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), M,
                                         n_id.data_ptr<int64_t>(), n_seg.data_ptr<int64_t>(), D, ptr.data_ptr<int64_t>(),
                                         vptr.data_ptr<int64_t>(), V, ws.data_ptr(), row_o.data_ptr<int64_t>(),
                                         col_o.data_ptr<int64_t>(), e_id.data_ptr<int64_t>(), stream),
                 "tsamd_ego_induced_write");
  Tensor out_rowptr = torch::empty({D + 1}, iopt);
  check_status(tsamd_ind2ptr(row_o.data_ptr<int64_t>(), D, K, out_rowptr.data_ptr<int64_t>(), stream), "tsamd_ind2ptr");
  return std::make_tuple(out_rowptr, col_o, n_id, e_id, ptr, root_n_id);
}

}  // namespace

// Entries of the segments `seg_idx` of (ptr, ind) whose index is in `map_idx` (ids of a space of M_map nodes):
// -> (position of the segment in seg_idx, position of the index in map_idx, position of the entry), in
// seg_idx order and stored order inside a segment.  Two host syncs.  (Homogeneous graphs: seg_idx == map_idx;
// a relation of a heterogeneous graph: destination nodes select the segments, source nodes the entries.)
// first_wins: a node listed twice in map_idx keeps its FIRST position (the map insert of the neighbour samplers,
// neighbor_sample_cpu.cpp:31, 195) instead of its last (the assignment of subgraph_cpu, saint_cpu.cpp:17-18)
std::tuple<Tensor, Tensor, Tensor> induced_entries_bipartite(Tensor seg_idx, Tensor map_idx, int64_t M_map, Tensor ptr,
                                                             Tensor ind, bool first_wins) {
  seg_idx = seg_idx.contiguous();
  map_idx = map_idx.contiguous();
  const int64_t n = map_idx.numel();
  auto iopt = ptr.options().requires_grad(false);
  Tensor assoc = torch::empty({M_map}, iopt), err = torch::empty({1}, iopt);
  const bool flip = first_wins && n > 1;  // last position in the reversed list = first position in the list
  const Tensor listed = flip ? map_idx.flip(0).contiguous() : map_idx;
  check_status(tsamd_subset_assoc(listed.data_ptr<int64_t>(), n, M_map, assoc.data_ptr<int64_t>(), err.data_ptr<int64_t>(),
                                  current_stream(ptr)),
               "tsamd_subset_assoc");
  if (flip) assoc = torch::where(assoc >= 0, (n - 1) - assoc, assoc);
  auto sel = select_segments(ptr, ind, seg_idx, true, true);  // sync 1 (raises on bad ids)
  Tensor seg = std::get<1>(sel), nbr = std::get<2>(sel), pos = std::get<3>(sel);
  MappedFilter filter = MappedFilter::count(nbr, assoc, torch::empty({1}, iopt));
  auto kept = filter.write(seg, read_words({filter.counter})[0]);  // sync 2
  return std::make_tuple(std::get<0>(kept), std::get<1>(kept), pos.index_select(0, std::get<2>(kept)));
}

}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_sample = torch::RegisterOperators()
                                  .op("torch_sparse::random_walk", &random_walk)
                                  .op("tsamd::random_walk_with_rand", &random_walk_with_rand)
                                  .op("torch_sparse::sample_adj", &sample_adj)
                                  .op("torch_sparse::relabel", &relabel)
                                  .op("torch_sparse::relabel_one_hop", &relabel_one_hop)
                                  .op("torch_sparse::saint_subgraph", &saint_subgraph)
                                  .op("torch_sparse::neighbor_sample", &neighbor_sample)
                                  .op("torch_sparse::ego_k_hop_sample_adj", &ego_k_hop_sample_adj);
