// torch operator glue, part 9: the relational (typed-edge) SpMM (csrc/rel_gemm.hip).  See ops_spmm.cpp for the
// conventions.
//
//   tsamd::spmm_rel(Tensor rowptr, Tensor col, Tensor? value, Tensor row, Tensor rel, Tensor? colptr, Tensor? csr2csc,
//                   Tensor x, Tensor weight, str reduce) -> Tensor
//
//   out[i, :] = sum over the entries e of row i of  value[e] * (x[col[e], :] @ weight[rel[e]])          reduce = 'sum'
//   'mean': the sum over the relations of the MEAN over the entries of every (row, relation) pair (R-GCN's default).
//
// Aggregate first, then one grouped product.  A pair is a distinct (row, relation); the plan is built per call:
//   tsamd_sort_coalesce of (row, rel) with the entry ids riding along -> pairptr [P + 1] over the sorted entries, the
//   permutation eperm, prow / prel of every pair;  tsamd_ind2ptr(prow) -> rowpairptr [M + 1];  tsamd_sort_coo of
//   (prel, prow) -> the relation-major order q of the pairs, tsamd_ind2ptr of its keys -> relptr [R + 1].
// One host sync: P and the range of rel travel back together.  Then
//   A  H = tsamd_spmm(pairptr, col[eperm], value[eperm], x)           [P, F]    sum or mean per pair
//   B  Y[q[t], :] = H[q[t], :] @ weight[g]   (tsamd_rel_gemm)         [P, Fo]   fp32
//   C  out = tsamd_segment_reduce(sum) of Y over rowpairptr, cast     [M, Fo]
// Backward (once; x and weight):
//   gH[q[t], :] = grad[prow[q[t]], :] @ weight[g]^T  (tsamd_rel_gemm, transposed; scaled by 1 / count for 'mean')
//   grad_x = the transposed sum-SpMM of gH: tsamd_spmm_permuted over (colptr, pair id of the entry, value, csr2csc)
//   grad_weight[g] = sum_t H[q[t], :]^T (outer) grad[prow[q[t]], :]   (tsamd_rel_wgrad)
// A 4-D weight [R, B, ci, co] is block-diagonal, weight[g] = diag of its B blocks (csrc/rel_blocks.hip): plan, A and C
// are shared, step B and the two backward products go to tsamd_rel_gemm_blocks / tsamd_rel_wgrad_blocks; B = 1 is the
// dense call on the squeezed weight.
#include "ops_common.h"

namespace tsamd_ops {
namespace {

inline const int64_t *lp(const Tensor &t) { return t.data_ptr<int64_t>(); }
inline int64_t *lp(Tensor &t) { return t.data_ptr<int64_t>(); }

void check_rel_args(const Tensor &rowptr, const Tensor &col, const OptTensor &value, const Tensor &row, const Tensor &rel,
                    const Tensor &x, const Tensor &weight, const std::string &reduce) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  check_index(row, "row");
  check_gpu(x, "x");
  check_gpu(weight, "weight");
  check_gpu(rel, "rel");
  TORCH_CHECK_VALUE(reduce == "sum" || reduce == "add" || reduce == "mean", "spmm_rel: reduce must be 'sum' or 'mean', got '",
                    reduce, "'");
  TORCH_CHECK_VALUE(x.dim() == 2, "spmm_rel: x must be [N, F], got ", x.dim(), " dimension(s); a batched x is not supported");
  TORCH_CHECK_VALUE(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16,
                    "spmm_rel: float32 or bfloat16 expected, got ", x.scalar_type());
  if (weight.dim() == 4) {  // block-diagonal: [R, B, ci, co]
    TORCH_CHECK_VALUE(weight.size(1) >= 1 && weight.size(2) >= 1 && weight.size(3) >= 1 &&
                          weight.size(1) * weight.size(2) == x.size(1),
                      "spmm_rel: a block-diagonal weight must be [R, B, ci, co] with B ci = ", x.size(1), ", got ",
                      weight.sizes());
  } else {
    TORCH_CHECK_VALUE(weight.dim() == 3 && weight.size(1) == x.size(1), "spmm_rel: weight must be [R, F, Fo] with F = ",
                      x.size(1), ", got ", weight.sizes());
  }
  TORCH_CHECK_VALUE(weight.scalar_type() == x.scalar_type(), "spmm_rel: weight and x differ in dtype: ",
                    weight.scalar_type(), " and ", x.scalar_type());
  const int64_t Fo = weight.dim() == 4 ? weight.size(1) * weight.size(3) : weight.size(2);
  TORCH_CHECK_VALUE(x.size(1) >= 1 && x.size(1) <= 512 && Fo >= 1 && Fo <= 512,
                    "spmm_rel: F and Fo must lie in 1 .. 512, got ", x.size(1), " and ", Fo);
  TORCH_CHECK_VALUE(weight.size(0) >= 1, "spmm_rel: weight holds no relation");
  TORCH_CHECK_VALUE(rel.scalar_type() == at::kLong && rel.dim() == 1 && rel.numel() == col.numel(),
                    "spmm_rel: rel must be an int64 tensor with one relation per entry ([", col.numel(), "]), got ",
                    rel.scalar_type(), " ", rel.sizes());
  TORCH_CHECK_VALUE(row.numel() == col.numel() && rowptr.numel() >= 1, "spmm_rel: row, col and rowptr do not match");
  TORCH_CHECK(x.get_device() == col.get_device() && x.get_device() == weight.get_device() &&
                  x.get_device() == rel.get_device(),
              "spmm_rel: x, weight, rel and the pattern must be on one device");
  if (value.has_value()) {
    const Tensor &v = value.value();
    check_gpu(v, "value");
    TORCH_CHECK_VALUE(v.dim() == 1 && v.size(0) == col.size(0), "spmm_rel: value must be [nnz], got ", v.sizes());
    TORCH_CHECK_VALUE(v.scalar_type() == x.scalar_type(), "spmm_rel: value and x differ in dtype: ", v.scalar_type(),
                      " and ", x.scalar_type());
    TORCH_CHECK_VALUE(!needs_grad(v), "spmm_rel: a value that requires a gradient is not supported");
  }
}

Tensor ind2ptr(const Tensor &ind, int64_t n) {
  Tensor ptr = torch::empty({n + 1}, ind.options());
  check_status(tsamd_ind2ptr(lp(ind), n, ind.numel(), lp(ptr), current_stream(ind)), "tsamd_ind2ptr");
  return ptr;
}

// one tsamd_rel_gemm (weight [R, *, *]) or tsamd_rel_gemm_blocks (weight [R, B, *, *]; K and N are B times its
// block sizes): out [n_dst, N] fp32, rows no item names are not written
Tensor rel_gemm(bool transposed, const Tensor &src, const Tensor &src_idx, const Tensor &dst_idx, const Tensor &relptr,
                const Tensor &weight, const Tensor &scale, int64_t n_dst, int64_t K, int64_t N) {
  const int64_t P = dst_idx.numel(), R = relptr.numel() - 1;
  const int dt = dtype_code(src);
  Tensor out = torch::empty({n_dst, N}, src.options().dtype(at::kFloat).requires_grad(false));
  if (weight.dim() == 4) {
    const int64_t B = weight.size(1);
    Tensor ws = workspace(tsamd_rel_gemm_blocks_workspace_bytes(dt, P, R, B, K / B, N / B), src);
    check_status(tsamd_rel_gemm_blocks(dt, transposed ? 1 : 0, src.data_ptr(), src.size(0), lp(src_idx), lp(dst_idx),
                                       lp(relptr), weight.data_ptr(), scale.defined() ? scale.data_ptr<float>() : nullptr,
                                       out.data_ptr<float>(), n_dst, P, R, B, K / B, N / B, ws.data_ptr(),
                                       (size_t)ws.numel(), current_stream(src)),
                 "tsamd_rel_gemm_blocks");
    return out;
  }
  Tensor ws = workspace(tsamd_rel_gemm_workspace_bytes(dt, P, R, K, N), src);
  check_status(tsamd_rel_gemm(dt, transposed ? 1 : 0, src.data_ptr(), src.size(0), lp(src_idx), lp(dst_idx), lp(relptr),
                              weight.data_ptr(), scale.defined() ? scale.data_ptr<float>() : nullptr,
                              out.data_ptr<float>(), n_dst, P, R, K, N, ws.data_ptr(), (size_t)ws.numel(),
                              current_stream(src)),
               "tsamd_rel_gemm");
  return out;
}

// Saved: col, value, colptr, csr2csc, weight, H, pairptr, eperm, prow, q, relptr.
class SpmmRelFunction : public torch::autograd::Function<SpmmRelFunction> {
 public:
  static Tensor forward(AutogradContext *ctx, Tensor rowptr_, Tensor col_, Tensor value_, Tensor row_, Tensor rel_,
                        OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor x_, Tensor weight_, bool has_value,
                        bool mean) {
    const bool has_csc = opt_colptr.has_value() && opt_csr2csc.has_value();
    TORCH_CHECK(!needs_grad(x_) || has_csc, "spmm_rel: the gradient with respect to x needs colptr and csr2csc");
    c10::hip::HIPGuard guard(x_.get_device());
    Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous(), row = row_.contiguous(), rel = rel_.contiguous();
    Tensor x = x_.detach().contiguous(), weight = weight_.detach().contiguous();
    Tensor value = has_value ? value_.detach().contiguous() : Tensor();
    const int64_t M = rowptr.numel() - 1, N = x.size(0), F = x.size(1), E = col.numel();
    const int64_t B = weight.dim() == 4 ? weight.size(1) : 0;  // 0: a dense [R, F, Fo] weight
    const int64_t R = weight.size(0), Fo = B ? B * weight.size(3) : weight.size(2);
    const int dt = dtype_code(x);
    void *stream = current_stream(x);
    const auto ids = col.options().requires_grad(false);
    ctx->saved_data["B"] = B;
    ctx->saved_data["has_value"] = has_value;
    ctx->saved_data["mean"] = mean;
    ctx->saved_data["P"] = (int64_t)0;
    ctx->saved_data["M"] = M;
    ctx->saved_data["N"] = N;
    Tensor none = torch::empty({0}, ids);
    if (E == 0 || M == 0) {
      ctx->save_for_backward({col, none, none, none, weight_, none, none, none, none, none, none});
      return torch::zeros({M, Fo}, x.options().requires_grad(false));
    }
    if (has_csc) {
      check_index(opt_colptr.value(), "colptr");
      check_index(opt_csr2csc.value(), "csr2csc");
      TORCH_CHECK(opt_csr2csc.value().numel() == E && opt_colptr.value().numel() == N + 1, "Input mismatch");
    }

    // the plan: pairs in (row, rel) order with the entry ids riding along
    Tensor row_t = torch::empty({E}, ids), rel_t = torch::empty({E}, ids), prow = torch::empty({E}, ids);
    Tensor prel = torch::empty({E}, ids), pairptr = torch::empty({E + 1}, ids), eperm = torch::empty({E}, ids);
    Tensor stats = torch::empty({5}, ids);  // counts [3], then the range of rel
    Tensor entry = torch::arange(E, ids);
    {
      Tensor ws = workspace(tsamd_sort_coalesce_workspace_bytes(E), x);
      check_status(tsamd_sort_coalesce(lp(row), lp(rel), E, M, R, lp(row_t), lp(rel_t), lp(prow), lp(prel), lp(pairptr),
                                       lp(stats), entry.data_ptr(), eperm.data_ptr(), 8, ws.data_ptr(), (size_t)ws.numel(),
                                       stream),
                   "tsamd_sort_coalesce");
    }
    auto range = rel.aminmax();
    stats.narrow(0, 3, 1).copy_(std::get<0>(range).reshape({1}));
    stats.narrow(0, 4, 1).copy_(std::get<1>(range).reshape({1}));
    const Tensor host = stats.cpu();  // the call's one host sync
    const int64_t P = host.data_ptr<int64_t>()[2];
    TORCH_CHECK_VALUE(host.data_ptr<int64_t>()[3] >= 0 && host.data_ptr<int64_t>()[4] < R,
                      "spmm_rel: rel must lie in [0, ", R, "), got values from ", host.data_ptr<int64_t>()[3], " to ",
                      host.data_ptr<int64_t>()[4]);
    TORCH_CHECK(P >= 1 && P <= E, "spmm_rel: the plan counted ", P, " pairs for ", E, " entries");
    pairptr = pairptr.narrow(0, 0, P + 1);
    prow = prow.narrow(0, 0, P).contiguous();
    prel = prel.narrow(0, 0, P).contiguous();
    Tensor rowpairptr = ind2ptr(prow, M);
    auto by_rel = sort_coo(prel, prow, R, M, true);  // (prel sorted, prow sorted, q)
    Tensor q = std::get<2>(by_rel);
    Tensor relptr = ind2ptr(std::get<0>(by_rel), R);

    // A: the existing SpMM over the pairs
    Tensor colp = col.index_select(0, eperm);
    Tensor valp = has_value ? value.index_select(0, eperm) : Tensor();
    Tensor H = torch::empty({P, F}, x.options().requires_grad(false));
    {
      const int red = mean ? TSAMD_MEAN : TSAMD_SUM;
      Tensor ws = workspace(tsamd_spmm_workspace_bytes(dt, red, 1, P, N, F, E), x);
      check_status(tsamd_spmm(dt, red, lp(pairptr), lp(colp), has_value ? valp.data_ptr() : nullptr, x.data_ptr(),
                              H.data_ptr(), nullptr, 1, P, N, F, E, ws.data_ptr(), (size_t)ws.numel(), stream),
                   "tsamd_spmm");
    }
    // B: the grouped product, C: the pairs of every row
    Tensor Y = rel_gemm(false, H, q, q, relptr, weight, Tensor(), P, F, Fo);
    Tensor out32 = torch::empty({M, Fo}, Y.options());
    check_status(tsamd_segment_reduce(TSAMD_F32, TSAMD_SUM, Y.data_ptr(), nullptr, lp(rowpairptr), M, Fo, out32.data_ptr(),
                                      stream),
                 "tsamd_segment_reduce");
    ctx->saved_data["P"] = P;
    ctx->save_for_backward({col, has_value ? value : none, opt_colptr.value_or(none), opt_csr2csc.value_or(none), weight_,
                            H, pairptr, eperm, prow, q, relptr});
    return out32.to(x.scalar_type());
  }

  static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
    const bool has_value = ctx->saved_data["has_value"].toBool(), mean = ctx->saved_data["mean"].toBool();
    const int64_t P = ctx->saved_data["P"].toInt(), M = ctx->saved_data["M"].toInt(), N = ctx->saved_data["N"].toInt();
    auto s = ctx->get_saved_variables();
    variable_list none(11);
    const bool want_x = ctx->needs_input_grad(7), want_w = ctx->needs_input_grad(8);
    if ((!want_x && !want_w) || !grad_outs[0].defined()) return none;
    TORCH_CHECK(!at::GradMode::is_enabled(), "spmm_rel: second-order gradients are not supported");
    Tensor weight = s[4].detach().contiguous();
    const int64_t B = ctx->saved_data["B"].toInt(), R = weight.size(0);
    const int64_t F = B ? B * weight.size(2) : weight.size(1), Fo = B ? B * weight.size(3) : weight.size(2);
    if (P == 0) {
      if (want_x) none[7] = torch::zeros({N, F}, weight.options());
      if (want_w) none[8] = torch::zeros_like(weight);
      return none;
    }
    c10::hip::HIPGuard guard(weight.get_device());
    Tensor col = s[0], value = s[1], colptr = s[2].contiguous(), csr2csc = s[3].contiguous(), H = s[5], pairptr = s[6],
           eperm = s[7], prow = s[8], q = s[9], relptr = s[10];
    const int64_t E = col.numel();
    const int dt = dtype_code(weight);
    void *stream = current_stream(weight);
    Tensor g = grad_outs[0].to(weight.scalar_type()).contiguous();
    Tensor prow_q = prow.index_select(0, q);  // the row of grad every item reads
    if (want_x) {
      Tensor scale;
      if (mean) scale = (pairptr.slice(0, 1) - pairptr.slice(0, 0, P)).to(at::kFloat).reciprocal_();
      Tensor gH = rel_gemm(true, g, prow_q, q, relptr, weight, scale, P, Fo, F);
      // the pair of every entry, in CSR order
      Tensor pair_sorted = torch::empty({E}, col.options());
      check_status(tsamd_ptr2ind(lp(pairptr), P, E, lp(pair_sorted), stream), "tsamd_ptr2ind");
      Tensor epair = torch::empty({E}, col.options());
      epair.index_copy_(0, eperm, pair_sorted);
      Tensor v32 = has_value ? value.to(at::kFloat).contiguous() : Tensor();
      Tensor gx = torch::empty({N, F}, gH.options());
      Tensor ws = workspace(tsamd_spmm_workspace_bytes(TSAMD_F32, TSAMD_SUM, 1, N, P, F, E), gH);
      check_status(tsamd_spmm_permuted(TSAMD_F32, TSAMD_SUM, lp(colptr), lp(epair), has_value ? v32.data_ptr() : nullptr,
                                       lp(csr2csc), gH.data_ptr(), gx.data_ptr(), nullptr, 1, N, P, F, E, ws.data_ptr(),
                                       (size_t)ws.numel(), stream),
                   "tsamd_spmm_permuted");
      none[7] = gx.to(weight.scalar_type());
    }
    if (want_w) {
      Tensor gw = torch::empty_like(weight, weight.options().requires_grad(false));
      if (B) {
        Tensor ws = workspace(tsamd_rel_wgrad_blocks_workspace_bytes(dt, P, R, B, F / B, Fo / B), weight);
        check_status(tsamd_rel_wgrad_blocks(dt, H.data_ptr(), P, lp(q), g.data_ptr(), M, lp(prow_q), lp(relptr),
                                            gw.data_ptr(), P, R, B, F / B, Fo / B, ws.data_ptr(), (size_t)ws.numel(),
                                            stream),
                     "tsamd_rel_wgrad_blocks");
      } else {
        Tensor ws = workspace(tsamd_rel_wgrad_workspace_bytes(dt, P, R, F, Fo), weight);
        check_status(tsamd_rel_wgrad(dt, H.data_ptr(), P, lp(q), g.data_ptr(), M, lp(prow_q), lp(relptr), gw.data_ptr(), P,
                                     R, F, Fo, ws.data_ptr(), (size_t)ws.numel(), stream),
                     "tsamd_rel_wgrad");
      }
      none[8] = gw;
    }
    return none;
  }
};

Tensor spmm_rel(Tensor rowptr, Tensor col, OptTensor value, Tensor row, Tensor rel, OptTensor colptr, OptTensor csr2csc,
                Tensor x, Tensor weight, std::string reduce) {
  check_rel_args(rowptr, col, value, row, rel, x, weight, reduce);
  if (weight.dim() == 4 && weight.size(1) == 1) weight = weight.squeeze(1);  // one block is the dense product
  return SpmmRelFunction::apply(rowptr, col, value.value_or(col), row, rel, colptr, csr2csc, x, weight, value.has_value(),
                                reduce == "mean");
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_spmm_rel = torch::RegisterOperators().op(
    "tsamd::spmm_rel(Tensor rowptr, Tensor col, Tensor? value, Tensor row, Tensor rel, Tensor? colptr, Tensor? csr2csc, "
    "Tensor x, Tensor weight, str reduce) -> Tensor",
    &spmm_rel);
