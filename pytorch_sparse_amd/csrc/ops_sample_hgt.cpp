// torch operator glue, part 3d: HGT budget sampling (csrc/cpu/hgt_sample_cpu.cpp).  See ops_spmm.cpp for the
// conventions, ops_sample.h for the steps the samplers share.
#include "ops_sample.h"

#include <algorithm>

namespace tsamd_ops {
namespace {

// ---- HGT budget sampling (csrc/cpu/hgt_sample_cpu.cpp) ----------------------------------------------------------------
edge_t split_relation(const rel_t &rel) {
  std::vector<std::string> parts;
  size_t start = 0;
  for (;;) {
    const size_t end = rel.find("__", start);
    parts.push_back(rel.substr(start, end == std::string::npos ? std::string::npos : end - start));
    if (end == std::string::npos) break;
    start = end + 2;
  }
  TORCH_CHECK(parts.size() == 3, "hgt_sample: relation key '", rel, "' is not of the form src__rel__dst");
  return std::make_tuple(parts[0], parts[1], parts[2]);
}

// what one node type carries through a call of hgt_sample (csrc/hgt_sample.hip): the dense budget / seen words, the
// candidate list, and the node list as one tensor per block (the inputs, then what every hop drew)
struct HgtType {
  Tensor word, cand;
  int64_t M = 0, tag = 0;
  int64_t C = 0;      // length of the candidate list as of the last read-back
  int64_t drawn = 0;  // candidates drawn so far (dead entries of the list)
  std::vector<Tensor> blocks;
  Tensor fresh;  // the newest block: what the next budget update expands
};

// torch_sparse::hgt_sample(Dict(str, Tensor) colptr_dict, Dict(str, Tensor) row_dict, Dict(str, Tensor) input_node_dict,
//     Dict(str, int[]) num_samples_dict, int num_hops)
//     -> (Dict(str, Tensor) node, Dict(str, Tensor) row, Dict(str, Tensor) col, Dict(str, Tensor) edge)
// (reference schema, csrc/hgt_sample.cpp; CPU-only there).  The node types are the keys of num_samples_dict, the
// relations those of colptr_dict (src__rel__dst, one CSC each).  Every type keeps a budget over its unseen nodes: a
// newly listed node w adds 1 / min(deg, 50) to every unseen source of its column (50 uniform entries of a longer
// column), per relation into w's type; a hop draws num_samples[t][hop] nodes of every type without replacement,
// sequentially proportional to budget^2, and expands them.  The edges are those of the (at most 50 per column)
// entries of the final lists' columns whose source is listed.  What the random draws do not decide is the reference's
// result; docs/design/widening.md lists the divergences.  Host read-backs: 3 + num_hops (the set-up's id maxima, one
// per budget update, two for the edges), whatever the number of types, relations, inputs and samples.
std::tuple<TensorDict, TensorDict, TensorDict, TensorDict> hgt_sample(
    const TensorDict &colptr_dict, const TensorDict &row_dict, const TensorDict &input_node_dict,
    const c10::Dict<node_t, std::vector<int64_t>> &num_samples_dict, int64_t num_hops) {
  std::vector<node_t> node_types;
  for (const auto &kv : num_samples_dict) {
    node_types.push_back(kv.key());
    TORCH_CHECK((int64_t)kv.value().size() >= num_hops, "num_samples_dict[", kv.key(), "] has fewer than num_hops entries");
    for (int64_t ell = 0; ell < num_hops; ++ell)
      TORCH_CHECK(kv.value()[ell] >= 0, "num_samples_dict[", kv.key(), "] has a negative entry");
  }
  std::sort(node_types.begin(), node_types.end());
  std::vector<rel_t> rels;  // ascending key order: the order of the draws' seeds
  std::vector<edge_t> edge_types;
  for (const auto &kv : colptr_dict) rels.push_back(kv.key());
  std::sort(rels.begin(), rels.end());
  for (const auto &rel : rels) {
    const edge_t et = split_relation(rel);
    TORCH_CHECK(num_samples_dict.contains(std::get<0>(et)), "hgt_sample: unknown node type ", std::get<0>(et), " in ", rel);
    TORCH_CHECK(num_samples_dict.contains(std::get<2>(et)), "hgt_sample: unknown node type ", std::get<2>(et), " in ", rel);
    TORCH_CHECK(row_dict.contains(rel), "hgt_sample: row_dict has no entry ", rel);
    edge_types.push_back(et);
  }
  for (const auto &kv : input_node_dict)
    TORCH_CHECK(num_samples_dict.contains(kv.key()), "hgt_sample: unknown node type ", kv.key(), " in input_node_dict");
  // id space of every type: one read-back, the relations' maxima remembered per graph (hetero_setup)
  HeteroSetup hs = hetero_setup(node_types, edge_types, colptr_dict, row_dict, input_node_dict, num_samples_dict);
  c10::hip::HIPGuard guard(hs.any.get_device());
  auto iopt = hs.any.options().requires_grad(false);
  void *stream = current_stream(hs.any);
  const int64_t kCap = TSAMD_HGT_MAX_NEIGHBORS;

  // device words, two per type: (length of the candidate list, #bad ids and other errors)
  Tensor state = torch::zeros({2 * (int64_t)node_types.size()}, iopt);
  std::map<node_t, HgtType> types;
  for (size_t i = 0; i < node_types.size(); ++i) {
    HgtType &ty = types[node_types[i]];
    ty.M = hs.num_nodes.at(node_types[i]);
    ty.tag = (int64_t)i;
    ty.word = torch::zeros({ty.M}, iopt);
    ty.cand = torch::empty({ty.M}, iopt);
    ty.fresh = input_node_dict.contains(node_types[i]) ? input_node_dict.at(node_types[i]).contiguous() : torch::empty({0}, iopt);
    if (ty.fresh.numel() > 0) ty.blocks.push_back(ty.fresh);
  }
  auto words = [&](HgtType &ty) { return reinterpret_cast<uint64_t *>(ty.word.data_ptr<int64_t>()); };
  auto st = [&](HgtType &ty) { return state.data_ptr<int64_t>() + 2 * ty.tag; };
  auto check_state = [&](const int64_t *h) {
    for (const auto &t : node_types) {
      HgtType &ty = types.at(t);
      TORCH_CHECK_INDEX(h[2 * ty.tag + 1] == 0, "index out of range: ", h[2 * ty.tag + 1], " node ids of type ", t,
                        " are outside [0, ", ty.M, ")");
      ty.C = h[2 * ty.tag];
    }
  };
  auto mark_seen = [&](HgtType &ty) {
    check_status(tsamd_hgt_seen(ty.fresh.data_ptr<int64_t>(), ty.fresh.numel(), ty.M, words(ty), st(ty) + 1, stream),
                 "tsamd_hgt_seen");
  };
  for (size_t r = 0; r < rels.size(); ++r)  // (an id space without ids and a non-empty row: every entry is negative)
    TORCH_CHECK_INDEX(types.at(std::get<0>(edge_types[r])).M > 0 || row_dict.at(rels[r]).numel() == 0,
                      "index out of range: row_dict[", rels[r], "] has negative entries only");
  const uint64_t seed0 = host_seed();
  uint64_t draw_no = 0;
  // the budget update for the newest block of every type.  The draws are not sized by a read-back: a column gives at
  // most 50, so F * 50 slots hold them and tsamd_hgt_budget_add walks the plan's segments itself; ONE transfer then
  // brings the candidate counters, the error words and the plans' bad-id counts.
  auto update_budget = [&]() {
    std::vector<Drawn> plans = plan_hop(rels, colptr_dict, row_dict, seed0, draw_no, [&](size_t r) {
      const bool none = row_dict.at(rels[r]).numel() == 0;
      return std::make_tuple(none ? Tensor() : types.at(std::get<2>(edge_types[r])).fresh, kCap, false);
    });
    if (plans.empty()) return;
    std::vector<Tensor> parts;
    for (Drawn &d : plans) {
      HgtType &src = types.at(std::get<0>(edge_types[d.rel]));
      d.T = d.F * kCap;  // an upper bound: the slots behind the plan's total stay unused
      draw_planned(d);
      check_status(tsamd_hgt_budget_add(d.out_ptr.data_ptr<int64_t>(), d.F, d.nbr.data_ptr<int64_t>(), src.M, words(src),
                                        src.cand.data_ptr<int64_t>(), src.cand.numel(), st(src), stream),
                   "tsamd_hgt_budget_add");
      parts.push_back(d.info);
    }
    parts.push_back(state);
    const std::vector<int64_t> host = read_words(parts);  // host sync: the update's one read-back
    for (size_t i = 0; i < plans.size(); ++i) check_plan_ids(plans[i], host[2 * i + 1], "node");
    check_state(host.data() + 2 * plans.size());
  };

  for (const auto &t : node_types) mark_seen(types.at(t));  // every input is seen before any budget is added
  if (num_hops > 0) update_budget();
  // a hop's draws: the race keys of every type that draws (tsamd_hgt_keys), ONE sort of all of them -- the type tag
  // rides on top of the key, and at mini-batch sizes a sort costs its launches, not what it moves --, then every type
  // takes the first `take` entries of its segment (tsamd_hgt_commit).  The key takes 32 bits + the bits of the type tag
  // above the id: when that and the bits of the largest id space exceed the sort's 64, every type sorts alone.
  int64_t max_M = 1;
  for (const auto &t : node_types) max_M = std::max(max_M, types.at(t).M);
  const int64_t n_tags = (int64_t)node_types.size();
  int key_bits = 32, id_bits = 0;
  while (((int64_t)1 << (key_bits - 32)) < n_tags) ++key_bits;
  while (id_bits < 63 && ((int64_t)1 << id_bits) < max_M) ++id_bits;
  const bool one_sort = key_bits + id_bits <= 64;
  const uint64_t select_seed = hgt_select_seed(seed0);
  for (int64_t ell = 0; ell < num_hops; ++ell) {
    std::vector<HgtType *> drawing;
    std::vector<int64_t> takes;
    int64_t total_C = 0;
    for (const auto &t : node_types) {
      HgtType &ty = types.at(t);
      const int64_t take = std::min<int64_t>(num_samples_dict.at(t)[ell], ty.C - ty.drawn);
      ty.fresh = torch::empty({take}, iopt);
      if (take == 0) continue;
      drawing.push_back(&ty);
      takes.push_back(take);
      total_C += ty.C;
    }
    if (one_sort && drawing.size() > 1) {
      Tensor keys = torch::empty({4, total_C}, iopt), perm = torch::empty({total_C}, iopt);  // key, id, sorted key, sorted id
      int64_t *key = keys.data_ptr<int64_t>(), *id = key + total_C, *key_s = id + total_C, *id_s = key_s + total_C;
      int64_t off = 0;
      for (HgtType *ty : drawing) {  // ascending tag: the order of the segments after the sort
        check_status(tsamd_hgt_keys(ty->cand.data_ptr<int64_t>(), ty->C, words(*ty), ty->M, select_seed, ell, ty->tag,
                                    key + off, id + off, stream),
                     "tsamd_hgt_keys");
        off += ty->C;
      }
      Tensor ws = workspace(tsamd_sort_coo_workspace_bytes(total_C), keys);
      check_status(tsamd_sort_coo(key, id, total_C, n_tags << 32, max_M, key_s, id_s, perm.data_ptr<int64_t>(), ws.data_ptr(),
                                  (size_t)ws.numel(), stream),
                   "tsamd_sort_coo");
      off = 0;
      for (size_t i = 0; i < drawing.size(); ++i) {
        HgtType *ty = drawing[i];
        check_status(tsamd_hgt_commit(key_s + off, id_s + off, takes[i], words(*ty), ty->M, ty->tag,
                                      ty->fresh.data_ptr<int64_t>(), st(*ty) + 1, stream),
                     "tsamd_hgt_commit");
        off += ty->C;
      }
    } else {
      for (size_t i = 0; i < drawing.size(); ++i) {
        HgtType *ty = drawing[i];
        Tensor ws = workspace(tsamd_hgt_select_workspace_bytes(ty->C), ty->word);
        check_status(tsamd_hgt_select(ty->cand.data_ptr<int64_t>(), ty->C, words(*ty), ty->M, takes[i], select_seed, ell,
                                      ty->tag, ty->fresh.data_ptr<int64_t>(), st(*ty) + 1, ws.data_ptr(),
                                      (size_t)ws.numel(), stream),
                     "tsamd_hgt_select");
      }
    }
    for (size_t i = 0; i < drawing.size(); ++i) {
      drawing[i]->blocks.push_back(drawing[i]->fresh);
      drawing[i]->drawn += takes[i];
    }
    if (ell < num_hops - 1) update_budget();
  }

  // the edges: per relation the (at most 50 per column) entries of the final dst list whose source is listed
  std::map<node_t, Tensor> samples;
  for (const auto &t : node_types) {
    HgtType &ty = types.at(t);
    samples[t] = ty.blocks.empty() ? torch::empty({0}, iopt) : (ty.blocks.size() == 1 ? ty.blocks[0] : torch::cat(ty.blocks));
  }
  std::vector<Drawn> plans = plan_hop(rels, colptr_dict, row_dict, seed0, draw_no, [&](size_t r) {
    const bool none = samples.at(std::get<0>(edge_types[r])).numel() == 0 || row_dict.at(rels[r]).numel() == 0;
    return std::make_tuple(none ? Tensor() : samples.at(std::get<2>(edge_types[r])), kCap, false);
  });
  read_plans(plans);  // host sync: the draws of all relations
  std::map<node_t, Tensor> assoc;  // node -> local id, a duplicate's LAST position (the reference assigns)
  std::vector<Tensor> segs, parts;
  std::vector<MappedFilter> filters;
  Tensor scratch_err = torch::empty({1}, iopt);
  for (Drawn &d : plans) {
    const node_t &src_t = std::get<0>(edge_types[d.rel]);
    HgtType &src = types.at(src_t);
    draw_planned(d);
    check_status(tsamd_hgt_check_ids(d.nbr.data_ptr<int64_t>(), d.T, src.M, st(src) + 1, stream), "tsamd_hgt_check_ids");
    if (!assoc.count(src_t)) {
      assoc[src_t] = torch::empty({src.M}, iopt);
      check_status(tsamd_subset_assoc(samples.at(src_t).data_ptr<int64_t>(), samples.at(src_t).numel(), src.M,
                                      assoc[src_t].data_ptr<int64_t>(), scratch_err.data_ptr<int64_t>(), stream),
                   "tsamd_subset_assoc");
    }
    segs.push_back(segment_ids(d.out_ptr, d.F, d.T));
    filters.push_back(MappedFilter::count(d.nbr, assoc[src_t], torch::zeros({1}, iopt)));
    parts.push_back(filters.back().counter);
  }
  parts.push_back(state);
  const std::vector<int64_t> host = read_words(parts);  // host sync: the kept entries of all relations + the error words
  check_state(host.data() + plans.size());
  std::map<rel_t, std::vector<Tensor>> rows, cols, edges;  // (a relation without a plan or a kept entry: empty tensors)
  for (size_t i = 0; i < plans.size(); ++i) {
    if (host[i] == 0) continue;
    auto kept = filters[i].write(segs[i], host[i]);
    const rel_t &rel = rels[plans[i].rel];
    cols[rel].push_back(std::get<0>(kept));
    rows[rel].push_back(std::get<1>(kept));
    edges[rel].push_back(plans[i].e.index_select(0, std::get<2>(kept)));
  }
  return pack_hetero(node_types, colptr_dict, samples, rows, cols, edges, hs.any, /*omit_empty_types=*/true);
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_sample_hgt = torch::RegisterOperators().op("torch_sparse::hgt_sample", &hgt_sample);
