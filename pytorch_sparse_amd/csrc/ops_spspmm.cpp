// torch operator glue, part 3: tsamd::spspmm, C = A * B on CSR operands (csrc/spspmm.hip), and its autograd in the
// value tensors (csrc/spspmm_bw.hip).  See ops_spmm.cpp for the conventions.
#include "ops_common.h"

namespace tsamd_ops {
namespace {

// C = A * B on CSR operands -> (rowptrC, colC, valueC); valueC is empty unless with_value.
// Count first, write once (csrc/spspmm.hip); two host syncs (size classes, nnz(C)) because the
// scratch of oversized rows and the output size are data dependent.
std::tuple<Tensor, Tensor, Tensor> spspmm_fw(Tensor rowptrA, Tensor colA, OptTensor valA,
                                             Tensor rowptrB, Tensor colB, OptTensor valB, int64_t N,
                                             bool with_value) {
  check_index(rowptrA, "rowptrA");
  check_index(colA, "colA");
  check_index(rowptrB, "rowptrB");
  check_index(colB, "colB");
  c10::hip::HIPGuard guard(rowptrA.get_device());
  rowptrA = rowptrA.contiguous();
  colA = colA.contiguous();
  rowptrB = rowptrB.contiguous();
  colB = colB.contiguous();
  auto vdtype = valA.has_value() ? valA.value().scalar_type()
                                 : (valB.has_value() ? valB.value().scalar_type() : at::kFloat);
  TORCH_CHECK(vdtype == at::kFloat || vdtype == at::kDouble,
              "spspmm: only float32 and float64 values are supported (got ", vdtype, ")");
  if (valA.has_value() && valB.has_value())
    TORCH_CHECK(valA.value().scalar_type() == valB.value().scalar_type(), "spspmm: dtype mismatch");
  Tensor va = valA.has_value() ? valA.value().contiguous() : Tensor();
  Tensor vb = valB.has_value() ? valB.value().contiguous() : Tensor();
  const int dt = vdtype == at::kFloat ? TSAMD_F32 : TSAMD_F64;
  const int64_t M = rowptrA.numel() - 1;
  TORCH_CHECK(rowptrB.numel() - 1 >= 0 && M >= 0, "spspmm: bad rowptr");
  auto iopt = rowptrA.options();
  auto vopt = iopt.dtype(vdtype);
  void *stream = current_stream(rowptrA);

  Tensor prod = torch::empty({M + 1}, iopt), bins = torch::empty({2 * M + 1}, iopt);
  Tensor stats = torch::empty({8}, iopt);
  Tensor colB32 = torch::empty({colB.numel()}, iopt.dtype(at::kInt));  // 32-bit copy for the gathers
  // what the three stages are handed, taken from the tensors once
  const int64_t *rpA = rowptrA.data_ptr<int64_t>(), *cA = colA.data_ptr<int64_t>();
  const int64_t *rpB = rowptrB.data_ptr<int64_t>();
  const void *pva = valA.has_value() ? va.data_ptr() : nullptr, *pvb = valB.has_value() ? vb.data_ptr() : nullptr;
  uint32_t *cb32 = reinterpret_cast<uint32_t *>(colB32.data_ptr<int32_t>());
  int64_t *pprod = prod.data_ptr<int64_t>(), *pbins = bins.data_ptr<int64_t>();
  check_status(tsamd_spspmm_plan(rpA, cA, rpB, colB.data_ptr<int64_t>(), colB.numel(), M, pprod, pbins, cb32,
                                 stats.data_ptr<int64_t>(), stream),
               "tsamd_spspmm_plan");
  Tensor h = stats.cpu();  // sync 1: grid sizes, workspace of the rows beyond the LDS capacity
  const int64_t *hs = h.data_ptr<int64_t>();
  const int64_t n_medium = hs[2], n_large = hs[3], P_large = hs[4];
  // the large-row path counts the products of a (row, column range) bin in 32-bit LDS words
  TORCH_CHECK(hs[5] < ((int64_t)1 << 31), "spspmm: a row of the product has ", hs[5],
              " intermediate products; rows of 2^31 or more are not supported");

  const size_t ws_bytes = tsamd_spspmm_workspace_bytes(dt, n_large, P_large, N);
  if (n_large > 0) {  // data dependent scratch: refuse politely instead of an allocator OOM
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      TORCH_CHECK((double)ws_bytes < 0.9 * (double)free_b, "spspmm: ", P_large, " intermediate products in ",
                  n_large, " rows beyond the LDS capacity need ~", (int64_t)((double)ws_bytes / 1e9),
                  " GB of scratch, more than the free device memory");
  }
  Tensor ws1 = workspace(ws_bytes, rowptrA);
  Tensor rowptrC = torch::zeros({M + 1}, iopt);  // nnzC in [0, M), scanned in place below
  int64_t *rpC = rowptrC.data_ptr<int64_t>();
  // with values: the large rows are binned once, values included (no third expansion in the numeric stage)
  const int bin_values = with_value ? 1 : 0;
  check_status(tsamd_spspmm_symbolic(dt, rpA, cA, pva, rpB, cb32, pvb, bin_values, M, N, pprod, pbins, n_medium, n_large,
                                     P_large, rpC, ws1.data_ptr(), (size_t)ws1.numel(), stream),
               "tsamd_spspmm_symbolic");
  Tensor total = torch::empty({1}, iopt);
  Tensor ws2 = workspace(tsamd_exclusive_scan_workspace_bytes(M + 1), rowptrA);
  check_status(tsamd_exclusive_scan_i64(rpC, rpC, M + 1, total.data_ptr<int64_t>(), ws2.data_ptr(),
                                        (size_t)ws2.numel(), stream),
               "tsamd_exclusive_scan_i64");
  const int64_t nnz = total.item<int64_t>();  // sync 2: the output size
  Tensor colC = torch::empty({nnz}, iopt);
  Tensor valC = with_value ? torch::empty({nnz}, vopt) : torch::empty({0}, vopt);
  check_status(tsamd_spspmm_numeric(dt, rpA, cA, pva, rpB, cb32, pvb, M, N, pprod, pbins, n_medium, n_large, P_large, rpC,
                                    colC.data_ptr<int64_t>(), with_value ? valC.data_ptr() : nullptr, bin_values,
                                    ws1.data_ptr(), (size_t)ws1.numel(), stream),
               "tsamd_spspmm_numeric");
  return std::make_tuple(rowptrC, colC, valC);
}

// One value gradient of C = A * B (csrc/spspmm_bw.hip, include/tsamd.h "SpSpMM value gradients"): plan, then the
// balanced kernel.  `stats` (device, 2 int64) is filled by plan(); run() wants its host copy.
struct SpspmmBwSide {
  int dt, side;
  Tensor segptr, segind, listptr, ptr;
  int64_t nrows, nseg;

  void plan(int dt_, int side_, const Tensor &segptr_, const Tensor &segind_, const Tensor &listptr_,
            int64_t *stats, void *stream) {
    dt = dt_, side = side_, segptr = segptr_, segind = segind_, listptr = listptr_;
    nrows = segptr.numel() - 1, nseg = segind.numel();
    ptr = torch::empty({nseg + 1}, segptr.options());
    Tensor ws = workspace(tsamd_spspmm_bw_plan_workspace_bytes(nseg), segptr);
    check_status(tsamd_spspmm_bw_plan(dt, side, segptr.data_ptr<int64_t>(), nrows, segind.data_ptr<int64_t>(), nseg,
                                      listptr.data_ptr<int64_t>(), ptr.data_ptr<int64_t>(), stats, ws.data_ptr(),
                                      (size_t)ws.numel(), stream),
                 "tsamd_spspmm_bw_plan");
  }

  Tensor run(const int64_t *hstats, const Tensor &list_ind, const Tensor &list_val, const Tensor &rowptrC,
             const Tensor &colC, const Tensor &gC, void *stream) {
    Tensor grad = torch::empty({nseg}, gC.options().requires_grad(false));
    Tensor ws = workspace((size_t)hstats[0], segptr);
    check_status(tsamd_spspmm_value_bw(dt, side, ptr.data_ptr<int64_t>(), hstats[1], segptr.data_ptr<int64_t>(), nrows,
                                       segind.data_ptr<int64_t>(), nseg, listptr.data_ptr<int64_t>(),
                                       list_ind.data_ptr<int64_t>(), list_val.defined() ? list_val.data_ptr() : nullptr,
                                       rowptrC.data_ptr<int64_t>(), colC.data_ptr<int64_t>(), gC.data_ptr(),
                                       grad.data_ptr(), ws.data_ptr(), (size_t)ws.numel(), stream),
                 "tsamd_spspmm_value_bw");
    return grad;
  }
};

// Autograd of tsamd::spspmm in the value tensors (first order; the backward records no graph, so a double
// backward raises).  The reference drops this gradient at C._values() (torch_sparse/matmul.py:102).
// Saved: the three patterns, both value tensors, A's column view when the caller had it.
class SpspmmFunction : public torch::autograd::Function<SpspmmFunction> {
 public:
  static variable_list forward(AutogradContext *ctx, Tensor rowptrA, Tensor colA, OptTensor valA, Tensor rowptrB,
                               Tensor colB, OptTensor valB, int64_t N, OptTensor colptrA, OptTensor csr2cscA) {
    auto out = spspmm_fw(rowptrA, colA, valA, rowptrB, colB, valB, N, true);
    Tensor rowptrC = std::get<0>(out), colC = std::get<1>(out), valC = std::get<2>(out);
    ctx->mark_non_differentiable({rowptrC, colC});
    const bool have_csc = colptrA.has_value() && csr2cscA.has_value();
    ctx->saved_data["has_a"] = valA.has_value();
    ctx->saved_data["has_b"] = valB.has_value();
    ctx->saved_data["have_csc"] = have_csc;
    // absent optionals are parked as `colA` (never read then)
    ctx->save_for_backward({rowptrA, colA, valA.value_or(colA), rowptrB, colB, valB.value_or(colA), rowptrC, colC,
                            have_csc ? colptrA.value() : colA, have_csc ? csr2cscA.value() : colA});
    return {rowptrC, colC, valC};
  }

  static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
    const bool has_a = ctx->saved_data["has_a"].toBool(), has_b = ctx->saved_data["has_b"].toBool();
    const bool have_csc = ctx->saved_data["have_csc"].toBool();
    auto s = ctx->get_saved_variables();
    Tensor rowptrA = s[0], colA = s[1], valA = s[2], rowptrB = s[3], colB = s[4], valB = s[5], rowptrC = s[6],
           colC = s[7];
    // only the sides this backward pass was asked for (torch.autograd.grad(valueC, [valueA]) skips gB); the edges
    // count the tensor arguments that were present: rowptrA, colA, [valA], rowptrB, colB, [valB]
    const bool want_a = has_a && needs_grad(valA) && ctx->needs_input_grad(2);
    const bool want_b = has_b && needs_grad(valB) && ctx->needs_input_grad(has_a ? 5 : 4);
    Tensor gA, gB;
    Tensor g = grad_outs[2];
    if (g.defined() && (want_a || want_b)) {
      c10::hip::HIPGuard guard(rowptrA.get_device());
      g = g.detach().contiguous();  // valueC.sum().backward() delivers a stride-0 expand
      const int dt = dtype_code(g);
      const int64_t M = rowptrA.numel() - 1, K = rowptrB.numel() - 1, nnzA = colA.numel();
      rowptrA = rowptrA.contiguous(), colA = colA.contiguous();
      rowptrB = rowptrB.contiguous(), colB = colB.contiguous();
      void *stream = current_stream(rowptrA);
      Tensor stats = torch::zeros({4}, rowptrA.options());
      SpspmmBwSide sa, sb;
      Tensor colptrA, rowA_t, valA_t;
      if (want_a) sa.plan(dt, 0, rowptrA, colA, rowptrB, stats.data_ptr<int64_t>(), stream);
      if (want_b) {  // the lists are the columns of A: (colptr, row and value in column order)
        Tensor rowA = torch::empty({nnzA}, rowptrA.options());
        check_status(tsamd_ptr2ind(rowptrA.data_ptr<int64_t>(), M, nnzA, rowA.data_ptr<int64_t>(), stream),
                     "tsamd_ptr2ind");
        Tensor perm;
        if (have_csc) {
          colptrA = s[8].contiguous();
          perm = s[9];
          rowA_t = rowA.index_select(0, perm);
        } else {
          auto sorted = sort_coo(colA, rowA, K, M, true);
          rowA_t = std::get<1>(sorted);
          perm = std::get<2>(sorted);
          colptrA = torch::empty({K + 1}, rowptrA.options());
          check_status(tsamd_ind2ptr(std::get<0>(sorted).data_ptr<int64_t>(), K, nnzA, colptrA.data_ptr<int64_t>(),
                                     stream),
                       "tsamd_ind2ptr");
        }
        TORCH_CHECK(colptrA.numel() == K + 1 && perm.numel() == nnzA, "spspmm: colptrA / csr2cscA do not fit A");
        if (has_a) valA_t = valA.detach().index_select(0, perm);
        sb.plan(dt, 1, rowptrB, colB, colptrA, stats.data_ptr<int64_t>() + 2, stream);
      }
      Tensor h = stats.cpu();  // the one sync: the number of products sizes the grid and the carry records
      const int64_t *hs = h.data_ptr<int64_t>();
      if (want_a)
        gA = sa.run(hs, colB, has_b ? valB.detach().contiguous() : Tensor(), rowptrC, colC, g, stream);
      if (want_b) gB = sb.run(hs + 2, rowA_t, valA_t, rowptrC, colC, g, stream);
    }
    return {Tensor(), Tensor(), gA, Tensor(), Tensor(), gB, Tensor(), Tensor(), Tensor()};
  }
};

// tsamd::spspmm: no value requires grad (or grad mode is off) -> the forward alone, no node.  colptrA / csr2cscA:
// the cached column view of A, used by the gradient of valB only (built in the backward when absent).
std::tuple<Tensor, Tensor, Tensor> spspmm(Tensor rowptrA, Tensor colA, OptTensor valA, Tensor rowptrB, Tensor colB,
                                          OptTensor valB, int64_t N, bool with_value, OptTensor colptrA,
                                          OptTensor csr2cscA) {
  const bool grad = with_value && torch::autograd::GradMode::is_enabled() &&
                    ((valA.has_value() && needs_grad(valA.value())) || (valB.has_value() && needs_grad(valB.value())));
  if (!grad) return spspmm_fw(rowptrA, colA, valA, rowptrB, colB, valB, N, with_value);
  auto out = SpspmmFunction::apply(rowptrA, colA, valA, rowptrB, colB, valB, N, colptrA, csr2cscA);
  return std::make_tuple(out[0], out[1], out[2]);
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_spspmm = torch::RegisterOperators().op(
    "tsamd::spspmm(Tensor rowptrA, Tensor colA, Tensor? valA, Tensor rowptrB, Tensor colB, "
    "Tensor? valB, int N, bool with_value, Tensor? colptrA=None, "
    "Tensor? csr2cscA=None) -> (Tensor, Tensor, Tensor)",
    &spspmm);
