// torch operator glue, part 8: the fused multi-aggregation (csrc/spmm_multi.hip).  See ops_spmm.cpp for the
// conventions.
//
//   tsamd::spmm_multi(Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor? csr2csc, Tensor? row, Tensor x,
//                     int mask) -> (Tensor out, Tensor argmin, Tensor argmax)
//
// out is [M, R, F], slot r the reduction with the r-th set bit of mask (tsamd_multi: sum 1, mean 2, min 4, max 8,
// var 16, std 32); argmin / argmax are [M, F] int64 entry ids (E: no winner), empty when min / max is not asked for.
// Differentiable once with respect to x when the CSC arrays are handed over (SparseTensor.matmul_multi does that when a
// gradient is being recorded, as storage_spmm does).  No new kernel of nnz size in the backward: with n the row's
// entries the gradient with respect to a product y_e of row r is c1[r] + c2[r] * y_e,
//   c1 = g_sum + g_mean / n - 2 g_var mean / n,   c2 = 2 g_var / n,   g_var including g_std / (2 std) (0 where std == 0),
// so the moments give grad_x = A^T c1 + x * ((A o A)^T c2): two sum-SpMMs through csr2csc (tsamd_spmm_permuted), the
// second only when var or std was asked for; min and max each add the deterministic pull of tsamd_spmm_minmax_bw_csc on
// their winners.  c1, c2 and the combination are [M, F]- and [N, F]-sized element-wise torch.
#include "ops_common.h"

namespace tsamd_ops {
namespace {

constexpr int64_t kMomentBits = TSAMD_MULTI_SUM | TSAMD_MULTI_MEAN | TSAMD_MULTI_VAR | TSAMD_MULTI_STD;
constexpr int64_t kAllBits = kMomentBits | TSAMD_MULTI_MIN | TSAMD_MULTI_MAX;

// slot of `bit` in an output of `mask`
int64_t slot_of(int64_t mask, int64_t bit) { return __builtin_popcountll(mask & (bit - 1)); }

void check_multi_args(const Tensor &rowptr, const Tensor &col, const OptTensor &value, const Tensor &x, int64_t mask) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  check_gpu(x, "x");
  TORCH_CHECK(x.dim() == 2, "spmm_multi: x must be [N, F], got ", x.dim(), " dimension(s); a batched x is not supported");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble || x.scalar_type() == at::kHalf ||
                  x.scalar_type() == at::kBFloat16,
              "spmm_multi: float32, float64, float16 or bfloat16 expected, got ", x.scalar_type());
  TORCH_CHECK(mask > 0 && (mask & ~kAllBits) == 0, "spmm_multi: mask must be a non-empty set of the six reduction bits, got ",
              mask);
  TORCH_CHECK(rowptr.numel() >= 1, "rowptr must not be empty");
  TORCH_CHECK(x.get_device() == col.get_device() && x.get_device() == rowptr.get_device(),
              "x and the pattern must be on one device");
  if (value.has_value()) {
    const Tensor &v = value.value();
    check_gpu(v, "value");
    TORCH_CHECK(v.dim() == 1 && v.size(0) == col.size(0), "value must be [nnz], got ", v.sizes());
    TORCH_CHECK(v.scalar_type() == x.scalar_type(), "value and x differ in dtype: ", v.scalar_type(), " and ",
                x.scalar_type());
    TORCH_CHECK(!needs_grad(v), "spmm_multi: a value that requires a gradient is not supported");
  }
}

// one forward on checked arguments -> (out [M, R, F], argmin, argmax)
std::tuple<Tensor, Tensor, Tensor> multi_run(const Tensor &rowptr_, const Tensor &col_, const OptTensor &value,
                                             const Tensor &x_, int64_t mask) {
  c10::hip::HIPGuard guard(x_.get_device());
  Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous(), x = x_.contiguous();
  Tensor v = value.has_value() ? value.value().contiguous() : Tensor();
  const int64_t M = rowptr.numel() - 1, N = x.size(0), F = x.size(1), E = col.numel();
  const int64_t R = __builtin_popcountll(mask);
  Tensor out = torch::empty({M, R, F}, x.options().requires_grad(false));
  const auto ids = rowptr.options().requires_grad(false);
  Tensor argmin = torch::empty({(mask & TSAMD_MULTI_MIN) ? M : 0, F}, ids);
  Tensor argmax = torch::empty({(mask & TSAMD_MULTI_MAX) ? M : 0, F}, ids);
  if (out.numel() == 0) return std::make_tuple(out, argmin, argmax);
  const int dt = dtype_code(x);
  Tensor ws = workspace(tsamd_spmm_multi_workspace_bytes(dt, (int)mask, M, F, E), x);
  check_status(tsamd_spmm_multi(dt, (int)mask, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                                v.defined() ? v.data_ptr() : nullptr, x.data_ptr(), out.data_ptr(), R * F, F,
                                argmin.numel() ? argmin.data_ptr<int64_t>() : nullptr,
                                argmax.numel() ? argmax.data_ptr<int64_t>() : nullptr, M, N, F, E, ws.data_ptr(),
                                (size_t)ws.numel(), current_stream(x)),
               "tsamd_spmm_multi");
  return std::make_tuple(out, argmin, argmax);
}

// A^T c through csr2csc, w the values in CSR order (undefined: ones) -> [N, F]
Tensor transposed_sum(const Tensor &colptr, const Tensor &row, const Tensor &csr2csc, const Tensor &w, const Tensor &c,
                      int64_t N) {
  const int64_t M = c.size(0), F = c.size(1), E = row.numel();
  Tensor out = torch::empty({N, F}, c.options().requires_grad(false));
  if (out.numel() == 0) return out;
  const int dt = dtype_code(c);
  Tensor ws = workspace(tsamd_spmm_workspace_bytes(dt, TSAMD_SUM, 1, N, M, F, E), c);
  check_status(tsamd_spmm_permuted(dt, TSAMD_SUM, colptr.data_ptr<int64_t>(), row.data_ptr<int64_t>(),
                                   w.defined() ? w.data_ptr() : nullptr, csr2csc.data_ptr<int64_t>(), c.data_ptr(),
                                   out.data_ptr(), nullptr, 1, N, M, F, E, ws.data_ptr(), (size_t)ws.numel(),
                                   current_stream(c)),
               "tsamd_spmm_permuted");
  return out;
}

// Saved: rowptr, col, value, colptr, csr2csc, row, x, full (the forward's output with the mean beside var / std),
// argmin, argmax.
class SpmmMultiFunction : public torch::autograd::Function<SpmmMultiFunction> {
 public:
  static variable_list forward(AutogradContext *ctx, Tensor rowptr, Tensor col, Tensor value, OptTensor opt_colptr,
                               OptTensor opt_csr2csc, OptTensor opt_row, Tensor x, bool has_value, int64_t mask) {
    const bool has_csc = opt_colptr.has_value() && opt_csr2csc.has_value() && opt_row.has_value();
    const bool grad = needs_grad(x);
    TORCH_CHECK(!grad || has_csc, "spmm_multi: the gradient with respect to x needs colptr, csr2csc and row");
    if (has_csc) {
      check_index(opt_colptr.value(), "colptr");
      check_index(opt_csr2csc.value(), "csr2csc");
      check_index(opt_row.value(), "row");
      TORCH_CHECK(opt_csr2csc.value().numel() == col.numel() && opt_row.value().numel() == col.numel() &&
                      opt_colptr.value().numel() == x.size(0) + 1,
                  "Input mismatch");
    }
    // the backward of var / std reads the row's mean: the same kernel writes it beside them
    const bool wants_var = (mask & (TSAMD_MULTI_VAR | TSAMD_MULTI_STD)) != 0;
    const int64_t run = grad && wants_var ? (mask | TSAMD_MULTI_MEAN) : mask;
    OptTensor v = has_value ? OptTensor(value) : std::nullopt;
    auto res = multi_run(rowptr, col, v, x, run);
    Tensor full = std::get<0>(res), out = full;
    if (run != mask) {
      std::vector<int64_t> keep;
      for (int64_t bit = 1; bit <= TSAMD_MULTI_STD; bit <<= 1)
        if (mask & bit) keep.push_back(slot_of(run, bit));
      out = full.index_select(1, torch::tensor(keep, rowptr.options()));
    }
    ctx->saved_data["has_value"] = has_value;
    ctx->saved_data["mask"] = mask;
    ctx->saved_data["run"] = run;
    ctx->save_for_backward({rowptr, col, value, opt_colptr.value_or(col), opt_csr2csc.value_or(col),
                            opt_row.value_or(col), x, grad ? full : Tensor(), std::get<1>(res), std::get<2>(res)});
    ctx->mark_non_differentiable({std::get<1>(res), std::get<2>(res)});
    return {out, std::get<1>(res), std::get<2>(res)};
  }

  static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
    const bool has_value = ctx->saved_data["has_value"].toBool();
    const int64_t mask = ctx->saved_data["mask"].toInt(), run = ctx->saved_data["run"].toInt();
    auto s = ctx->get_saved_variables();
    Tensor rowptr = s[0].contiguous(), col = s[1].contiguous(), value = s[2], colptr = s[3].contiguous(),
           csr2csc = s[4].contiguous(), row = s[5].contiguous(), x = s[6].contiguous(), full = s[7], argmin = s[8],
           argmax = s[9];
    variable_list none(9);
    if (!needs_grad(s[6]) || !grad_outs[0].defined()) return none;
    TORCH_CHECK(!at::GradMode::is_enabled(), "spmm_multi: second-order gradients are not supported");
    c10::hip::HIPGuard guard(x.get_device());
    const auto T = x.scalar_type();
    const auto opmath = T == at::kDouble ? at::kDouble : at::kFloat;
    const int64_t M = rowptr.numel() - 1, N = x.size(0), F = x.size(1), E = col.numel();
    Tensor g = grad_outs[0];
    Tensor v = has_value ? value.detach().contiguous() : Tensor();
    auto slice = [&](const Tensor &t, int64_t of, int64_t bit) { return t.select(1, slot_of(of, bit)).to(opmath); };
    Tensor n = (rowptr.slice(0, 1) - rowptr.slice(0, 0, M)).to(opmath).clamp_min_(1).unsqueeze(1);
    Tensor c1, c2;
    auto add = [](Tensor &acc, const Tensor &t) { acc = acc.defined() ? acc + t : t; };
    if (mask & TSAMD_MULTI_SUM) add(c1, slice(g, mask, TSAMD_MULTI_SUM));
    if (mask & TSAMD_MULTI_MEAN) add(c1, slice(g, mask, TSAMD_MULTI_MEAN) / n);
    Tensor g_var;
    if (mask & TSAMD_MULTI_VAR) add(g_var, slice(g, mask, TSAMD_MULTI_VAR));
    if (mask & TSAMD_MULTI_STD) {
      Tensor std = slice(full, run, TSAMD_MULTI_STD);
      Tensor gs = slice(g, mask, TSAMD_MULTI_STD) / (2 * std);
      add(g_var, torch::where(std > 0, gs, torch::zeros_like(gs)));
    }
    if (g_var.defined()) {
      c2 = 2 * g_var / n;
      add(c1, -(c2 * slice(full, run, TSAMD_MULTI_MEAN)));
    }
    Tensor grad_x;
    if (E == 0 || N * F == 0) {
      grad_x = torch::zeros_like(x);
    } else {
      if (c1.defined()) add(grad_x, transposed_sum(colptr, row, csr2csc, v, c1.to(T).contiguous(), N));
      if (c2.defined()) {
        Tensor v2 = has_value ? v * v : Tensor();
        add(grad_x, x.detach() * transposed_sum(colptr, row, csr2csc, v2, c2.to(T).contiguous(), N));
      }
      const int dt = dtype_code(x);
      for (int64_t bit : {(int64_t)TSAMD_MULTI_MIN, (int64_t)TSAMD_MULTI_MAX}) {
        if (!(mask & bit)) continue;
        Tensor gm = g.select(1, slot_of(mask, bit)).contiguous();
        Tensor part = torch::empty_like(x, x.options().requires_grad(false));
        Tensor ws = workspace(tsamd_spmm_minmax_bw_csc_workspace_bytes(dt, 1, M, N, F, E), x);
        const Tensor &arg = bit == TSAMD_MULTI_MIN ? argmin : argmax;
        check_status(tsamd_spmm_minmax_bw_csc(dt, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                                              has_value ? v.data_ptr() : nullptr, x.data_ptr(), gm.data_ptr(),
                                              arg.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                              csr2csc.data_ptr<int64_t>(), row.data_ptr<int64_t>(), nullptr,
                                              part.data_ptr(), 1, M, N, F, E, ws.data_ptr(), (size_t)ws.numel(),
                                              current_stream(x)),
                     "tsamd_spmm_minmax_bw_csc");
        add(grad_x, part);
      }
    }
    none[6] = grad_x;
    return none;
  }
};

std::tuple<Tensor, Tensor, Tensor> spmm_multi(Tensor rowptr, Tensor col, OptTensor value, OptTensor colptr,
                                              OptTensor csr2csc, OptTensor row, Tensor x, int64_t mask) {
  check_multi_args(rowptr, col, value, x, mask);
  auto r = SpmmMultiFunction::apply(rowptr, col, value.value_or(col), colptr, csr2csc, row, x, value.has_value(), mask);
  return std::make_tuple(r[0], r[1], r[2]);
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_spmm_multi = torch::RegisterOperators().op(
    "tsamd::spmm_multi(Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor? csr2csc, Tensor? row, "
    "Tensor x, int mask) -> (Tensor, Tensor, Tensor)",
    &spmm_multi);
