// torch operator glue, part 10: SpMM over fp8 (e4m3fn) features with row scales (csrc/spmm_q8.hip).  See ops_spmm.cpp
// for the conventions.
//
//   tsamd::spmm_q8(Tensor rowptr, Tensor col, Tensor? value, Tensor xq, Tensor? scale, str reduce, bool bf16_out)
//       -> Tensor            out [M, F] float32, or bfloat16 with bf16_out
//   tsamd::quantize_rows(Tensor x) -> (Tensor xq, Tensor scale)
//
// Neither is differentiable: the features are constants of a run, and nothing is recorded.
#include "ops_common.h"

namespace tsamd_ops {
namespace {

Tensor spmm_q8(Tensor rowptr_, Tensor col_, OptTensor value, Tensor xq_, OptTensor scale, std::string reduce,
               bool bf16_out) {
  check_index(rowptr_, "rowptr");
  check_index(col_, "col");
  check_gpu(xq_, "xq");
  TORCH_CHECK(xq_.scalar_type() == at::kFloat8_e4m3fn, "spmm_q8: xq must be float8_e4m3fn, got ", xq_.scalar_type());
  TORCH_CHECK(xq_.dim() == 2, "spmm_q8: xq must be [N, F], got ", xq_.dim(), " dimension(s)");
  TORCH_CHECK(xq_.size(1) <= 1024, "spmm_q8: F must be at most 1024, got ", xq_.size(1));
  TORCH_CHECK(rowptr_.numel() >= 1, "rowptr must not be empty");
  const int red = reduce_code(reduce);
  TORCH_CHECK(red == TSAMD_SUM || red == TSAMD_MEAN, "spmm_q8: reduce must be 'sum' or 'mean'");
  TORCH_CHECK(xq_.get_device() == col_.get_device() && xq_.get_device() == rowptr_.get_device(),
              "xq and the pattern must be on one device");
  const int64_t M = rowptr_.numel() - 1, N = xq_.size(0), F = xq_.size(1), E = col_.numel();
  Tensor v, s;
  if (value.has_value()) {
    check_gpu(value.value(), "value");
    TORCH_CHECK(value.value().dim() == 1 && value.value().size(0) == E, "value must be [nnz], got ",
                value.value().sizes());
    TORCH_CHECK(value.value().scalar_type() == at::kFloat, "spmm_q8: value must be float32, got ",
                value.value().scalar_type());
    TORCH_CHECK(!needs_grad(value.value()), "spmm_q8: a value that requires a gradient is not supported");
    v = value.value().contiguous();
  }
  if (scale.has_value()) {
    check_gpu(scale.value(), "scale");
    TORCH_CHECK(scale.value().dim() == 1 && scale.value().size(0) == N && scale.value().scalar_type() == at::kFloat,
                "spmm_q8: scale must be a float32 tensor of [", N, "]");
    s = scale.value().contiguous();
  }
  c10::hip::HIPGuard guard(xq_.get_device());
  Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous(), xq = xq_.contiguous();
  const auto odt = bf16_out ? at::kBFloat16 : at::kFloat;
  Tensor out = torch::empty({M, F}, xq.options().dtype(odt).requires_grad(false));
  if (out.numel() == 0) return out;
  const int dt = bf16_out ? TSAMD_BF16 : TSAMD_F32;
  Tensor ws = workspace(tsamd_spmm_q8_workspace_bytes(dt, M, F, E), xq);
  check_status(tsamd_spmm_q8(dt, red, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                             v.defined() ? v.data_ptr<float>() : nullptr, xq.data_ptr(),
                             s.defined() ? s.data_ptr<float>() : nullptr, out.data_ptr(), M, N, F, E, ws.data_ptr(),
                             (size_t)ws.numel(), current_stream(xq)),
               "tsamd_spmm_q8");
  return out;
}

std::tuple<Tensor, Tensor> quantize_rows(Tensor x_) {
  check_gpu(x_, "x");
  TORCH_CHECK(x_.dim() == 2, "quantize_rows: x must be [N, F], got ", x_.dim(), " dimension(s)");
  TORCH_CHECK(x_.scalar_type() == at::kFloat || x_.scalar_type() == at::kBFloat16 || x_.scalar_type() == at::kHalf,
              "quantize_rows: float32, bfloat16 or float16 expected, got ", x_.scalar_type());
  c10::hip::HIPGuard guard(x_.get_device());
  Tensor x = x_.detach().contiguous();
  const int64_t N = x.size(0), F = x.size(1);
  Tensor xq = torch::empty({N, F}, x.options().dtype(at::kFloat8_e4m3fn).requires_grad(false));
  Tensor scale = torch::empty({N}, x.options().dtype(at::kFloat).requires_grad(false));
  if (N == 0) return std::make_tuple(xq, scale);
  check_status(tsamd_quantize_rows(dtype_code(x), x.data_ptr(), xq.data_ptr(), scale.data_ptr<float>(), N, F,
                                   current_stream(x)),
               "tsamd_quantize_rows");
  return std::make_tuple(xq, scale);
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_q8 =
    torch::RegisterOperators()
        .op("tsamd::spmm_q8(Tensor rowptr, Tensor col, Tensor? value, Tensor xq, Tensor? scale, str reduce, "
            "bool bf16_out) -> Tensor",
            &spmm_q8)
        .op("tsamd::quantize_rows(Tensor x) -> (Tensor, Tensor)", &quantize_rows);
