// torch operator boundary of the MI355X sparse-matmul hot path.
//
// Registers the reference's operator names with the reference's schemas
// (csrc/spmm.cpp:344-348, csrc/convert.cpp:46-48, csrc/version.cpp:40-41 of
// rusty1s/pytorch_sparse) on top of the C-ABI in include/tsamd.h:
//
//   torch_sparse::spmm_sum (Tensor? row, Tensor rowptr, Tensor col, Tensor? value,
//                           Tensor? colptr, Tensor? csr2csc, Tensor mat) -> Tensor
//   torch_sparse::spmm_mean(Tensor? row, Tensor rowptr, Tensor col, Tensor? value,
//                           Tensor? rowcount, Tensor? colptr, Tensor? csr2csc, Tensor mat) -> Tensor
//   torch_sparse::spmm_min / spmm_max(Tensor rowptr, Tensor col, Tensor? value, Tensor mat)
//                                                                      -> (Tensor, Tensor)
//   torch_sparse::ind2ptr(Tensor ind, int M) / ptr2ind(Tensor ptr, int E) -> Tensor
//   torch_sparse::cuda_version() -> int
//
// Like the reference, autograd lives inside the op (torch::autograd::Function) and the
// kernels run on the current stream without synchronising.  Unlike the reference there is
// no CPU branch: tensors must live on the GPU, anything else raises.
#include "ops_common.h"
#include "ops_spmm_state.h"

namespace tsamd_ops {
namespace {

// ---- the forward's arguments, once ----------------------------------------------------------------------
// B, M, N, K, E of a product; mat.dim() >= 2
struct SpmmDims {
  int64_t B, M, N, K, E;
};
SpmmDims spmm_dims(const Tensor &rowptr, const Tensor &col, const Tensor &mat) {
  const int64_t N = mat.size(-2), K = mat.size(-1);
  return {(N * K) > 0 ? mat.numel() / (N * K) : 1, rowptr.numel() - 1, N, K, col.numel()};
}

// The argument checks of spmm_cpu.cpp:12-24 / spmm_cuda.cu:96-109, in the reference's order.
void check_spmm_args(const Tensor &rowptr, const Tensor &col, const OptTensor &opt_value, const Tensor &mat) {
  check_gpu(rowptr, "rowptr");
  check_gpu(col, "col");
  if (opt_value.has_value()) check_gpu(opt_value.value(), "value");
  check_gpu(mat, "mat");
  TORCH_CHECK(rowptr.dim() == 1 && col.dim() == 1, "Input mismatch");
  TORCH_CHECK(rowptr.scalar_type() == at::kLong && col.scalar_type() == at::kLong, "rowptr and col must be int64");
  if (opt_value.has_value()) {
    TORCH_CHECK(opt_value.value().dim() == 1, "Input mismatch");
    TORCH_CHECK(opt_value.value().size(0) == col.size(0), "Input mismatch");
    TORCH_CHECK(opt_value.value().scalar_type() == mat.scalar_type(), "expected scalar type ",
                mat.scalar_type(), " but found ", opt_value.value().scalar_type());
  }
  TORCH_CHECK(mat.dim() >= 2, "Input mismatch");
}

// What a forward hands to the C-ABI, from checked arguments: the contiguous operands, the sizes, the codes, and the
// outputs.  Winners of min / max: int64 ids (the API's arg_out), int32 ids where the caller keeps them for its own
// backward only and they fit, or none (the caller brings records).
enum class ArgIds { Wide, NarrowIfFits, None };
struct SpmmShape : SpmmDims {
  Tensor rowptr, col, mat;
  OptTensor value;
  int dt, red;
  Tensor out;
  OptTensor arg_out;
  bool arg32 = false;
  const int64_t *rp() const { return rowptr.data_ptr<int64_t>(); }
  const int64_t *cp() const { return col.data_ptr<int64_t>(); }
  int64_t *arg64() const { return arg_out.has_value() && !arg32 ? arg_out.value().data_ptr<int64_t>() : nullptr; }
};
SpmmShape spmm_shape(const Tensor &rowptr, const Tensor &col, const OptTensor &opt_value, const Tensor &mat, int red,
                     ArgIds ids) {
  SpmmShape s;
  s.mat = mat.contiguous();
  s.rowptr = rowptr.contiguous();
  s.col = col.contiguous();
  if (opt_value.has_value()) s.value = opt_value.value().contiguous();
  static_cast<SpmmDims &>(s) = spmm_dims(s.rowptr, s.col, s.mat);
  auto sizes = s.mat.sizes().vec();
  sizes[s.mat.dim() - 2] = s.M;
  s.out = torch::empty(sizes, s.mat.options().requires_grad(false));
  s.red = red;
  const bool minmax = red == TSAMD_MIN || red == TSAMD_MAX;
  s.arg32 = minmax && ids == ArgIds::NarrowIfFits && s.E < ((int64_t)1 << 31);
  if (minmax && ids != ArgIds::None)
    s.arg_out = torch::empty(sizes, s.arg32 ? s.rowptr.options().dtype(at::kInt) : s.rowptr.options());
  s.dt = dtype_code(s.mat);
  return s;
}

// One forward on checked arguments: exactly one C-ABI call.
// arg32: min / max winners as int32 ids (callers that keep them for their own backward only, tsamd.h)
// opt_perm: entries through a permutation (the CSC view in the backward)
// copy: the operand cache's buffer (spmm_fw_cached); copy_valid: it holds this operand's copy already
std::tuple<Tensor, OptTensor> spmm_run(const Tensor &rowptr, const Tensor &col, const OptTensor &opt_value,
                                       const Tensor &mat, int red, const OptTensor &opt_perm, bool arg32,
                                       const Tensor &copy = Tensor(), bool copy_valid = false) {
  c10::hip::HIPGuard guard(rowptr.get_device());
  const ArgIds ids = arg32 && !opt_perm.has_value() ? ArgIds::NarrowIfFits : ArgIds::Wide;
  const SpmmShape s = spmm_shape(rowptr, col, opt_value, mat, red, ids);
  void *stream = current_stream(s.mat);
  Tensor ws = workspace(copy.defined() ? tsamd_spmm_cached_workspace_bytes(s.dt, red, s.B, s.M, s.N, s.K, s.E)
                                       : tsamd_spmm_workspace_bytes(s.dt, red, s.B, s.M, s.N, s.K, s.E),
                        s.mat);
  void *w = ws.data_ptr(), *cbuf = copy.defined() ? copy.data_ptr() : nullptr;
  const size_t wb = (size_t)ws.numel(), cbytes = copy.defined() ? (size_t)copy.numel() : 0;
  if (s.arg32) {
    check_status(tsamd_spmm_minmax_arg32(s.dt, red, s.rp(), s.cp(), ptr_or_null(s.value), s.mat.data_ptr(),
                                         s.out.data_ptr(), s.arg_out.value().data_ptr<int32_t>(), s.B, s.M, s.N, s.K, s.E,
                                         w, wb, cbuf, cbytes, copy_valid ? 1 : 0, stream),
                 "tsamd_spmm_minmax_arg32");
  } else if (opt_perm.has_value()) {
    check_index(opt_perm.value(), "perm");
    TORCH_CHECK(opt_perm.value().numel() == s.E, "Input mismatch");
    Tensor perm = opt_perm.value().contiguous();
    check_status(tsamd_spmm_permuted(s.dt, red, s.rp(), s.cp(), ptr_or_null(s.value), perm.data_ptr<int64_t>(),
                                     s.mat.data_ptr(), s.out.data_ptr(), s.arg64(), s.B, s.M, s.N, s.K, s.E, w, wb,
                                     stream),
                 "tsamd_spmm_permuted");
  } else if (copy.defined()) {
    check_status(tsamd_spmm_cached(s.dt, red, s.rp(), s.cp(), ptr_or_null(s.value), s.mat.data_ptr(), s.out.data_ptr(),
                                   s.arg64(), s.B, s.M, s.N, s.K, s.E, w, wb, cbuf, cbytes, copy_valid ? 1 : 0, stream),
                 "tsamd_spmm_cached");
  } else {
    // the plain product: with the pattern's hints where it keeps any (built at the first sighting, reused from then on)
    const auto hints = pattern_hints_for(rowptr, col, s.dt, red, s.B, s.M, s.N, s.K, s.E, s.mat, stream);
    if (hints.second != 0) {
      const int st = tsamd_spmm_hinted(s.dt, red, s.rp(), s.cp(), ptr_or_null(s.value), s.mat.data_ptr(), s.out.data_ptr(),
                                       s.arg64(), s.B, s.M, s.N, s.K, s.E, w, wb, hints.first.data_ptr(), hints.second,
                                       stream);
      if (st != TSAMD_OK && hints.second == 1) pattern_hints_drop(hints.first);
      check_status(st, "tsamd_spmm_hinted");
    } else {
      check_status(tsamd_spmm(s.dt, red, s.rp(), s.cp(), ptr_or_null(s.value), s.mat.data_ptr(), s.out.data_ptr(),
                              s.arg64(), s.B, s.M, s.N, s.K, s.E, w, wb, stream),
                   "tsamd_spmm");
    }
  }
  return std::make_tuple(s.out, s.arg_out);
}

std::tuple<Tensor, OptTensor> spmm_fw(const Tensor &rowptr, const Tensor &col, const OptTensor &opt_value,
                                      const Tensor &mat, const std::string &reduce,
                                      const OptTensor &opt_perm = std::nullopt, bool arg32 = false) {
  check_spmm_args(rowptr, col, opt_value, mat);
  return spmm_run(rowptr, col, opt_value, mat, reduce_code(reduce), opt_perm, arg32);
}

// the forward of the registered ops: tsamd_spmm, or tsamd_spmm_cached when this product copies its operand
std::tuple<Tensor, OptTensor> spmm_fw_cached(const Tensor &rowptr, const Tensor &col, const OptTensor &opt_value,
                                             const Tensor &mat_in, const std::string &reduce, bool arg32 = false) {
  const int red = reduce_code(reduce);
  // the shapes tsamd_spmm_cached takes as they are; which of them copy their operand is the kernel side's decision
  bool shaped = operand_cache_enabled() && mat_in.defined() && mat_in.device().is_cuda() && mat_in.dim() >= 2 &&
                mat_in.is_contiguous() && rowptr.device().is_cuda() && rowptr.dim() == 1 && col.dim() == 1 &&
                col.is_contiguous() && rowptr.is_contiguous() &&
                (reinterpret_cast<uintptr_t>(mat_in.data_ptr()) % 16) == 0;
  if (shaped) {
    const at::ScalarType t = mat_in.scalar_type();
    shaped = t == at::kFloat || t == at::kDouble || t == at::kHalf || t == at::kBFloat16 || t == at::kInt || t == at::kLong;
  }
  if (shaped) {
    const SpmmDims d = spmm_dims(rowptr, col, mat_in);
    const int dt = dtype_code(mat_in);
    const size_t cache_bytes = tsamd_spmm_operand_cache_bytes(dt, red, d.B, d.M, d.N, d.K, d.E);
    if (cache_bytes != 0) {
      check_spmm_args(rowptr, col, opt_value, mat_in);  // (before the entry is re-armed: a refused call leaves it alone)
      c10::hip::HIPGuard guard(rowptr.get_device());
      const OperandCopy copy = operand_cache_copy(col, mat_in, dt, red, d.E, cache_bytes);  // (locked until the return)
      if (copy.buf.defined())
        return spmm_run(rowptr, col, opt_value, mat_in, red, std::nullopt, arg32, copy.buf, copy.valid);
    }
  }
  return spmm_fw(rowptr, col, opt_value, mat_in, reduce, std::nullopt, arg32);
}

Tensor spmm_value_bw(const Tensor &row, const Tensor &rowptr, const Tensor &col, Tensor mat,
                     Tensor grad, const std::string &reduce) {
  check_gpu(rowptr, "rowptr");
  check_gpu(mat, "mat");
  check_gpu(grad, "grad");
  c10::hip::HIPGuard guard(rowptr.get_device());
  mat = mat.contiguous();
  grad = grad.contiguous();
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  check_index(row, "row");
  Tensor rp = rowptr.contiguous(), c = col.contiguous(), r = row.contiguous();
  const SpmmDims d = spmm_dims(rp, c, mat);
  Tensor out = torch::empty({d.E}, grad.options().requires_grad(false));
  check_status(tsamd_spmm_value_bw(dtype_code(mat), reduce_code(reduce), r.data_ptr<int64_t>(),
                                   rp.data_ptr<int64_t>(), c.data_ptr<int64_t>(),
                                   mat.data_ptr(), grad.data_ptr(), out.data_ptr(), d.B, grad.size(-2), d.N, d.K, d.E,
                                   current_stream(mat)),
               "tsamd_spmm_value_bw");
  return out;
}

// The per-edge weights of grad_mat = A^T * grad_out in CSC order (row_t = row[csr2csc]): value[csr2csc] for sum,
// value[csr2csc] / max(rowcount[row_t], 1) for mean (rowcount given) -- its reciprocal count alone without values --
// or none.  t: the dtype of the product.
OptTensor csc_weights(const OptTensor &value, const Tensor &csr2csc, const OptTensor &rowcount, const Tensor &row_t,
                      at::ScalarType t) {
  if (!rowcount.has_value())
    return value.has_value() ? OptTensor(value.value().detach().index_select(0, csr2csc)) : std::nullopt;
  Tensor cnt = rowcount.value().index_select(0, row_t).to(t).clamp_min_(1);
  return value.has_value() ? value.value().detach().index_select(0, csr2csc).div_(cnt) : cnt.reciprocal_();
}

// ---- sum / mean ---------------------------------------------------------------------------
// One Function serves both: `mean` selects the divisor handling in both directions.
// Saved tensors: row, rowptr, col, value, rowcount, colptr, csr2csc, mat.
class SpmmAddFunction : public torch::autograd::Function<SpmmAddFunction> {
 public:
  static variable_list forward(AutogradContext *ctx, OptTensor opt_row, Tensor rowptr, Tensor col,
                               Tensor value, OptTensor opt_rowcount, OptTensor opt_colptr,
                               OptTensor opt_csr2csc, Tensor mat, bool has_value, bool mean, bool owned) {
    if (has_value && needs_grad(value)) TORCH_CHECK(opt_row.has_value(), "Argument `row` is missing");
    if (needs_grad(mat)) {
      TORCH_CHECK(opt_row.has_value(), "Argument `row` is missing");
      if (mean) TORCH_CHECK(opt_rowcount.has_value(), "Argument `rowcount` is missing");
      TORCH_CHECK(opt_colptr.has_value(), "Argument `colptr` is missing");
      TORCH_CHECK(opt_csr2csc.has_value(), "Argument `csr2csc` is missing");
    }
    OptTensor v = has_value ? OptTensor(value) : std::nullopt;
    Tensor out = std::get<0>(spmm_fw_cached(rowptr, col, v, mat, mean ? "mean" : "sum"));
    ctx->saved_data["has_value"] = has_value;
    ctx->saved_data["mean"] = mean;
    ctx->saved_data["owned"] = owned;
    // absent optionals are parked as `col` (any tensor will do; they are never read then)
    ctx->save_for_backward({opt_row.value_or(col), rowptr, col, value, opt_rowcount.value_or(col),
                            opt_colptr.value_or(col), opt_csr2csc.value_or(col), mat});
    return {out};
  }

  static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
    const bool has_value = ctx->saved_data["has_value"].toBool();
    const bool mean = ctx->saved_data["mean"].toBool();
    const bool owned = ctx->saved_data["owned"].toBool();
    Tensor grad_out = grad_outs[0];
    auto s = ctx->get_saved_variables();
    Tensor row = s[0], rowptr = s[1], col = s[2], value = s[3], rowcount = s[4], colptr = s[5],
           csr2csc = s[6], mat = s[7];

    Tensor grad_value, grad_mat;
    if (has_value && needs_grad(value))
      grad_value = spmm_value_bw(row, rowptr, col, mat, grad_out, mean ? "mean" : "sum");

    if (needs_grad(mat)) {
      // grad_mat = A^T * grad_out: the CSC arrays are the CSR of A^T; per-edge weights are
      // value (sum) or value / max(deg(row), 1) (mean) in CSC order.
      const OptTensor v = has_value ? OptTensor(value) : std::nullopt;
      // the pattern's kept CSC row ids, if any, and with them the values of a sum (mean divides its weights in place: it
      // gathers its own): one call, one lock
      const CscView kept = owned ? pattern_cache_csc_view(row, csr2csc, v, has_value && !mean) : CscView();
      if (mean) {
        Tensor row_t = kept.row_t.defined() ? kept.row_t : row.index_select(0, csr2csc);
        OptTensor w = csc_weights(v, csr2csc, rowcount, row_t, mat.scalar_type());
        grad_mat = std::get<0>(spmm_fw(colptr, row_t, w, grad_out, "sum"));
      } else if (kept.row_t.defined()) {
        // the pattern came back: its CSC row ids are at hand, only the values are gathered (one ATen gather)
        OptTensor w = has_value ? OptTensor(kept.value_t) : std::nullopt;
        grad_mat = std::get<0>(spmm_fw(colptr, kept.row_t, w, grad_out, "sum"));
      } else {
        // sum: the kernel reads (row, value) THROUGH csr2csc -- no row.index_select(0, csr2csc) /
        // value.index_select(0, csr2csc) temporaries as in the reference (spmm.cpp:104-106)
        OptTensor w = has_value ? OptTensor(value.detach()) : std::nullopt;
        grad_mat = std::get<0>(spmm_fw(colptr, row, w, grad_out, "sum", csr2csc));
      }
    }
    return {Tensor(), Tensor(), Tensor(), grad_value, Tensor(), Tensor(), Tensor(), grad_mat,
            Tensor(), Tensor(), Tensor()};
  }
};

// ---- min / max ----------------------------------------------------------------------------
// With the CSC arrays of the matrix (colptr, csr2csc, row -- SparseTensor.matmul hands them over when a
// gradient w.r.t. `mat` is wanted, exactly as it does for sum) the backward is the atomic-free pull of
// tsamd_spmm_minmax_bw_csc; the bare reference op (rowptr, col, value, mat) keeps the scatter kernel.
class SpmmMinMaxFunction : public torch::autograd::Function<SpmmMinMaxFunction> {
 public:
  static variable_list forward(AutogradContext *ctx, Tensor rowptr, Tensor col, Tensor value,
                               Tensor mat, bool has_value, bool is_max, OptTensor opt_colptr,
                               OptTensor opt_csr2csc, OptTensor opt_row, bool arg32) {
    OptTensor v = has_value ? OptTensor(value) : std::nullopt;
    const bool has_csc = opt_colptr.has_value() && opt_csr2csc.has_value() && opt_row.has_value();
    // Round 6: when the winners stay inside this node (arg32) and the pull backward is going to run (CSC arrays handed
    // over, a gradient w.r.t. mat recorded), the forward leaves the pull's winner RECORDS instead of ids
    // (tsamd_spmm_minmax_records: the merge kernel writes them where the winners sit in registers) and the backward
    // starts at the masked sum: configs[2] forward + backward 2.26 -> 2.15 ms, gradients bit-identical
    // (profiles/r06_ab_fwd_winrec.md).  Only when the records (32 bytes per entry up to 128 features, 48 up to 256) are at
    // most three times the ids they replace (4 bytes per output element) -- they are what the node holds until the backward.
    Tensor records;
    bool use_records = false;
    // (grad mode is off inside a Function's forward; the front-end hands the CSC arrays over only when it was on)
    if (arg32 && has_csc && needs_grad(mat) && !operand_cache_enabled() &&
        mat.device().is_cuda() && mat.dim() >= 2 && rowptr.dim() == 1 && col.dim() == 1 &&
        (mat.scalar_type() == at::kFloat || mat.scalar_type() == at::kHalf || mat.scalar_type() == at::kBFloat16) &&
        (!has_value || value.scalar_type() == mat.scalar_type()) && opt_row.value().numel() == col.numel() &&
        !stream_is_capturing(current_stream(mat))) {
      const SpmmDims d = spmm_dims(rowptr, col, mat);
      const bool value_grad_ok = !(has_value && needs_grad(value)) || (d.K * (int64_t)mat.element_size()) % 16 == 0;
      use_records = d.M > 0 && d.E > 0 && value_grad_ok &&
                    tsamd_spmm_minmax_records_in_forward(dtype_code(mat), d.B, d.M, d.K, d.E) == 1 &&
                    tsamd_spmm_minmax_records_bytes(d.B, d.K, d.E) <= (size_t)(3 * 4 * d.B * d.M * d.K);
    }
    Tensor out, arg_out;
    if (use_records) {
      check_index(rowptr, "rowptr");
      check_index(col, "col");
      check_index(opt_row.value(), "row");
      c10::hip::HIPGuard guard(mat.get_device());
      const SpmmShape s = spmm_shape(rowptr, col, v, mat, is_max ? TSAMD_MAX : TSAMD_MIN, ArgIds::None);
      Tensor r = opt_row.value().contiguous();
      if (has_value) TORCH_CHECK(value.dim() == 1 && value.size(0) == s.E, "Input mismatch");
      out = s.out;
      records = torch::empty({(int64_t)(tsamd_spmm_minmax_records_bytes(s.B, s.K, s.E) / 4)},
                             s.rowptr.options().dtype(at::kInt));
      Tensor ws = workspace(tsamd_spmm_minmax_records_workspace_bytes(s.dt, s.red, s.B, s.M, s.N, s.K, s.E), s.mat);
      check_status(tsamd_spmm_minmax_records(s.dt, s.red, s.rp(), s.cp(), ptr_or_null(s.value), s.mat.data_ptr(),
                                             out.data_ptr(), r.data_ptr<int64_t>(),
                                             reinterpret_cast<uint32_t *>(records.data_ptr<int32_t>()), s.B, s.M, s.N, s.K,
                                             s.E, ws.data_ptr(), (size_t)ws.numel(), current_stream(s.mat)),
                   "tsamd_spmm_minmax_records");
      arg_out = records;  // (what this mode returns in the ids' place: the caller asked not to see them)
    } else {
      auto res = spmm_fw_cached(rowptr, col, v, mat, is_max ? "max" : "min", arg32);
      out = std::get<0>(res);
      arg_out = std::get<1>(res).value();
    }
    if (has_csc) {
      check_index(opt_colptr.value(), "colptr");
      check_index(opt_csr2csc.value(), "csr2csc");
      check_index(opt_row.value(), "row");
      TORCH_CHECK(opt_csr2csc.value().numel() == col.numel() && opt_row.value().numel() == col.numel() &&
                      opt_colptr.value().numel() == mat.size(-2) + 1,
                  "Input mismatch");
    }
    ctx->saved_data["has_value"] = has_value;
    ctx->saved_data["has_csc"] = has_csc;
    ctx->saved_data["records"] = use_records;
    // the reference saves {col, value, mat, arg_out} (spmm.cpp:199); rowptr is kept as well so that
    // grad_value can be accumulated row by row (tsamd.h)
    ctx->save_for_backward({col, value, mat, arg_out, rowptr, opt_colptr.value_or(col),
                            opt_csr2csc.value_or(col), opt_row.value_or(col)});
    ctx->mark_non_differentiable({arg_out});
    return {out, arg_out};
  }

  // Which C-ABI entry a backward calls.  Only Scatter uses atomics (its grad_mat depends on their order); the three
  // pulls are deterministic.
  enum class Route { Records, PullIds32, PullIds64, Scatter };

  static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
    const bool has_value = ctx->saved_data["has_value"].toBool();
    const bool has_csc = ctx->saved_data["has_csc"].toBool();
    Tensor grad_out = grad_outs[0].contiguous();
    auto s = ctx->get_saved_variables();
    Tensor col = s[0].contiguous(), value = s[1].contiguous(), mat = s[2].contiguous(),
           arg_out = s[3].contiguous(), rowptr = s[4].contiguous();
    const bool want_value = has_value && needs_grad(value);
    const bool want_mat = needs_grad(mat);
    Tensor grad_value, grad_mat;
    if (!want_value && !want_mat)
      return {Tensor(), Tensor(), grad_value, grad_mat, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
    c10::hip::HIPGuard guard(mat.get_device());
    const SpmmDims d = spmm_dims(rowptr, col, mat);
    const int64_t B = d.B, M = grad_out.size(-2), N = d.N, K = d.K, E = d.E;
    const int dt = dtype_code(mat);
    // The pull is deterministic and faster for grad_mat alone (configs[2]: 1.36 vs 2.47 ms).  With grad_value as
    // well it pays a masked SDDMM where the scatter kernel gets the value gradient fused: WHICH of the two wins
    // depends on the row size, and the front-end decides that BEFORE the forward -- it hands the CSC arrays over
    // exactly when it wants the pull (pytorch_sparse_amd/tensor.py: storage_spmm).
    // The route, from what the C-ABI decides on (csrc/spmm_bw.hip: plan_minmax_csc, table in
    // docs/design/spmm_backward.md): the pull kernels hold 32-bit ids; int32 winners give grad_value only as the masked
    // SDDMM (16-byte packets), otherwise they are widened for the row-parallel kernel, which reads int64 ids.
    const bool records = ctx->saved_data["records"].toBool();  // the forward left the pull's winner records (see forward)
    Tensor colptr, csr2csc, row;
    if (records || (has_csc && want_mat)) {
      colptr = s[5].contiguous();
      csr2csc = s[6].contiguous();
      row = s[7].contiguous();
    }
    // The records route makes grad_value only as the masked SDDMM (16-byte packets) and has no ids to fall back on: an
    // operand that is contiguous but not 16-byte aligned (a view into a larger buffer) is copied into a fresh, aligned
    // allocation first.  The forward's gate has already kept rows that are no whole packets away.
    if (records && want_value) {
      if ((uintptr_t)grad_out.data_ptr() % 16 != 0) grad_out = grad_out.clone(at::MemoryFormat::Contiguous);
      if ((uintptr_t)mat.data_ptr() % 16 != 0) mat = mat.clone(at::MemoryFormat::Contiguous);
    }
    const bool narrow = arg_out.scalar_type() == at::kInt;
    const bool fits32 = N < ((int64_t)1 << 32) && M < ((int64_t)1 << 32) && E < ((int64_t)1 << 32) && K < ((int64_t)1 << 31);
    const bool packets16 = row.defined() && row.data_ptr() != nullptr && (K * (int64_t)mat.element_size()) % 16 == 0 &&
                           (uintptr_t)mat.data_ptr() % 16 == 0 && (uintptr_t)grad_out.data_ptr() % 16 == 0;
    Route route = Route::Scatter;  // no CSC arrays (the bare op), or sizes beyond the pull kernels' 32-bit ids
    if (records)
      route = Route::Records;
    else if (has_csc && want_mat && fits32)
      route = narrow && E < ((int64_t)1 << 31) && (!want_value || packets16) ? Route::PullIds32 : Route::PullIds64;

    if (want_value) grad_value = torch::empty({E}, mat.options().requires_grad(false));
    if (want_mat || route == Route::Records)  // (the records entry always writes grad_mat)
      grad_mat = torch::empty_like(mat, mat.options().requires_grad(false));
    if (narrow && (route == Route::PullIds64 || route == Route::Scatter)) arg_out = arg_out.to(at::kLong);
    Tensor ws = workspace(route == Route::Records   ? tsamd_spmm_minmax_bw_csc_records_workspace_bytes(dt, B, M, N, K, E)
                          : route == Route::Scatter ? tsamd_spmm_minmax_bw_workspace_bytes(dt, B, N, K, E)
                                                    : tsamd_spmm_minmax_bw_csc_workspace_bytes(dt, B, M, N, K, E),
                          mat);
    auto ids = [](const Tensor &t) { return t.defined() ? t.data_ptr<int64_t>() : nullptr; };
    const int64_t *rp = ids(rowptr), *cp = ids(col), *ccp = ids(colptr), *perm = ids(csr2csc), *rw = ids(row);
    const void *vp = has_value ? value.data_ptr() : nullptr, *x = mat.data_ptr(), *g = grad_out.data_ptr();
    void *gv = want_value ? grad_value.data_ptr() : nullptr, *gm = grad_mat.defined() ? grad_mat.data_ptr() : nullptr;
    void *w = ws.data_ptr(), *stream = current_stream(mat);
    const size_t wb = (size_t)ws.numel();
    // an UNSUPPORTED from the chosen entry means the rule above and plan_minmax_csc disagree: an error like any other
    switch (route) {
      case Route::Records:
        check_status(tsamd_spmm_minmax_bw_csc_records(dt, rp, cp, has_value ? 1 : 0, x, g,
                                                      reinterpret_cast<const uint32_t *>(arg_out.data_ptr<int32_t>()), ccp,
                                                      perm, rw, gv, gm, B, M, N, K, E, w, wb, stream),
                     "tsamd_spmm_minmax_bw_csc_records");
        if (!want_mat) grad_mat = Tensor();
        break;
      case Route::PullIds32:
        check_status(tsamd_spmm_minmax_bw_csc_arg32(dt, rp, cp, vp, x, g, arg_out.data_ptr<int32_t>(), ccp, perm, rw, gv, gm,
                                                    B, M, N, K, E, w, wb, stream),
                     "tsamd_spmm_minmax_bw_csc_arg32");
        break;
      case Route::PullIds64:
        check_status(tsamd_spmm_minmax_bw_csc(dt, rp, cp, vp, x, g, arg_out.data_ptr<int64_t>(), ccp, perm, rw, gv, gm, B, M,
                                              N, K, E, w, wb, stream),
                     "tsamd_spmm_minmax_bw_csc");
        break;
      case Route::Scatter:
        check_status(tsamd_spmm_minmax_bw(dt, rp, cp, vp, x, g, arg_out.data_ptr<int64_t>(), gv, gm, B, M, N, K, E, w, wb,
                                          stream),
                     "tsamd_spmm_minmax_bw");
        break;
    }
    return {Tensor(), Tensor(), grad_value, grad_mat, Tensor(), Tensor(), Tensor(), Tensor(), Tensor(), Tensor()};
  }
};

// ---- relabelled ("channel-camping free") layout, end to end (include/tsamd.h) -----------------
// position of every id of `ids` in a relabelled [n, *] matrix; ids == None: the whole map [n]
Tensor relabel_ids(OptTensor ids, int64_t n, Tensor like) {
  check_gpu(like, "like");
  c10::hip::HIPGuard guard(like.get_device());
  Tensor src;
  int64_t count = n;
  if (ids.has_value()) {
    check_index(ids.value(), "ids");
    src = ids.value().contiguous();
    count = src.numel();
  }
  Tensor out = torch::empty({count}, like.options().dtype(at::kLong).requires_grad(false));
  check_status(tsamd_relabel_ids(ids.has_value() ? src.data_ptr<int64_t>() : nullptr, count, n,
                                 out.data_ptr<int64_t>(), current_stream(like)),
               "tsamd_relabel_ids");
  return out;
}

std::tuple<Tensor, OptTensor> spmm_relabelled_fw(const Tensor &rowptr, const Tensor &col_h,
                                                 const OptTensor &opt_value, const Tensor &mat_h,
                                                 const std::string &reduce) {
  check_index(rowptr, "rowptr");
  check_index(col_h, "col_h");
  check_gpu(mat_h, "mat");
  TORCH_CHECK(mat_h.dim() >= 2, "Input mismatch");
  if (opt_value.has_value()) {
    check_gpu(opt_value.value(), "value");
    TORCH_CHECK(opt_value.value().dim() == 1 && opt_value.value().size(0) == col_h.size(0), "Input mismatch");
    TORCH_CHECK(opt_value.value().scalar_type() == mat_h.scalar_type(), "expected scalar type ",
                mat_h.scalar_type(), " but found ", opt_value.value().scalar_type());
  }
  c10::hip::HIPGuard guard(rowptr.get_device());
  const SpmmShape s = spmm_shape(rowptr, col_h, opt_value, mat_h, reduce_code(reduce), ArgIds::Wide);
  Tensor ws = workspace(tsamd_spmm_relabelled_workspace_bytes(s.dt, s.red, s.B, s.M, s.N, s.K, s.E), s.mat);
  check_status(tsamd_spmm_relabelled(s.dt, s.red, s.rp(), s.cp(), ptr_or_null(s.value), s.mat.data_ptr(), s.out.data_ptr(),
                                     s.arg64(), s.B, s.M, s.N, s.K, s.E, ws.data_ptr(), (size_t)ws.numel(),
                                     current_stream(s.mat)),
               "tsamd_spmm_relabelled");
  return std::make_tuple(s.out, s.arg_out);
}

// sum / mean in the relabelled layout with both gradients; the backward works in the same layout
// (grad_out arrives relabelled over M, grad_mat leaves relabelled over N).
// Saved: row, rowptr, col_h, value, rowcount, colptr, csr2csc, mat_h.
class SpmmRelabelledFunction : public torch::autograd::Function<SpmmRelabelledFunction> {
 public:
  static variable_list forward(AutogradContext *ctx, OptTensor opt_row, Tensor rowptr, Tensor col_h,
                               Tensor value, OptTensor opt_rowcount, OptTensor opt_colptr,
                               OptTensor opt_csr2csc, Tensor mat_h, bool has_value, bool mean) {
    if ((has_value && needs_grad(value)) || needs_grad(mat_h)) {
      TORCH_CHECK(opt_row.has_value(), "Argument `row` is missing");
      if (mean) TORCH_CHECK(opt_rowcount.has_value(), "Argument `rowcount` is missing");
    }
    if (needs_grad(mat_h)) {
      TORCH_CHECK(opt_colptr.has_value(), "Argument `colptr` is missing");
      TORCH_CHECK(opt_csr2csc.has_value(), "Argument `csr2csc` is missing");
    }
    OptTensor v = has_value ? OptTensor(value) : std::nullopt;
    Tensor out = std::get<0>(spmm_relabelled_fw(rowptr, col_h, v, mat_h, mean ? "mean" : "sum"));
    ctx->saved_data["has_value"] = has_value;
    ctx->saved_data["mean"] = mean;
    ctx->save_for_backward({opt_row.value_or(col_h), rowptr, col_h, value, opt_rowcount.value_or(col_h),
                            opt_colptr.value_or(col_h), opt_csr2csc.value_or(col_h), mat_h});
    return {out};
  }

  static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
    const bool has_value = ctx->saved_data["has_value"].toBool();
    const bool mean = ctx->saved_data["mean"].toBool();
    Tensor grad_h = grad_outs[0].contiguous();
    auto s = ctx->get_saved_variables();
    Tensor row = s[0], rowptr = s[1], col_h = s[2], value = s[3], rowcount = s[4], colptr = s[5],
           csr2csc = s[6], mat_h = s[7];
    const int64_t M = rowptr.numel() - 1;
    Tensor grad_value, grad_mat;
    if (has_value && needs_grad(value)) {
      // SDDMM over the pattern with both operands gathered at relabelled positions
      Tensor row_h = relabel_ids(row, M, row);
      grad_value = spmm_value_bw(row_h, rowptr, col_h, mat_h, grad_h, "sum");
      if (mean) grad_value = grad_value / rowcount.index_select(0, row).to(grad_value.scalar_type()).clamp_min_(1);
    }
    if (needs_grad(mat_h)) {
      Tensor row_t = row.index_select(0, csr2csc);
      OptTensor w = csc_weights(has_value ? OptTensor(value) : std::nullopt, csr2csc,
                                mean ? OptTensor(rowcount) : std::nullopt, row_t, mat_h.scalar_type());
      grad_mat = std::get<0>(spmm_relabelled_fw(colptr, relabel_ids(row_t, M, row_t), w, grad_h, "sum"));
    }
    return {Tensor(), Tensor(), Tensor(), grad_value, Tensor(), Tensor(), Tensor(), grad_mat,
            Tensor(), Tensor()};
  }
};

// (out_h, arg_out_h or an empty tensor).  min / max are forward only in this layout.
std::tuple<Tensor, Tensor> spmm_relabelled(OptTensor opt_row, Tensor rowptr, Tensor col_h,
                                           OptTensor opt_value, OptTensor opt_rowcount,
                                           OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor mat_h,
                                           std::string reduce) {
  const int red = reduce_code(reduce);
  if (red == TSAMD_MIN || red == TSAMD_MAX) {
    TORCH_CHECK(!needs_grad(mat_h) && !(opt_value.has_value() && needs_grad(opt_value.value())),
                "spmm_relabelled: min / max have no backward in the relabelled layout; use "
                "torch.ops.torch_sparse.spmm_", reduce, " on the plain layout for training");
    auto r = spmm_relabelled_fw(rowptr, col_h, opt_value, mat_h, reduce);
    return std::make_tuple(std::get<0>(r), std::get<1>(r).value());
  }
  Tensor value = opt_value.value_or(col_h);
  Tensor out = SpmmRelabelledFunction::apply(opt_row, rowptr, col_h, value, opt_rowcount, opt_colptr,
                                             opt_csr2csc, mat_h, opt_value.has_value(),
                                             red == TSAMD_MEAN)[0];
  return std::make_tuple(out, torch::empty({0}, rowptr.options()));
}

// dst = src[idx] for a 2-D row-major matrix (send buffer of the sharded SpMM's row exchange)
Tensor gather_rows(Tensor src, Tensor idx) {
  check_gpu(src, "src");
  check_index(idx, "idx");
  TORCH_CHECK(src.dim() == 2, "gather_rows: src must be 2-D");
  c10::hip::HIPGuard guard(src.get_device());
  src = src.contiguous();
  idx = idx.contiguous();
  Tensor out = torch::empty({idx.numel(), src.size(1)}, src.options().requires_grad(false));
  check_status(tsamd_gather_rows(src.data_ptr(), idx.data_ptr<int64_t>(), out.data_ptr(), idx.numel(),
                                 src.size(0), src.size(1) * (int64_t)src.element_size(),
                                 current_stream(src)),
               "tsamd_gather_rows");
  return out;
}

// ---- registered entry points (reference signatures) -----------------------------------------
// owned: the index arrays belong to a SparseStorage (SparseTensor.matmul): the backward may keep row[csr2csc] (and
// value[csr2csc] of non-trainable weights) across calls -- see PatternCache in ops_spmm_state.cpp
Tensor spmm_add(OptTensor opt_row, Tensor rowptr, Tensor col, OptTensor opt_value, OptTensor opt_rowcount,
                OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor mat, bool mean, bool owned) {
  Tensor value = opt_value.value_or(col);
  return SpmmAddFunction::apply(opt_row, rowptr, col, value, opt_rowcount, opt_colptr, opt_csr2csc, mat,
                                opt_value.has_value(), mean, owned)[0];
}

Tensor spmm_sum(OptTensor opt_row, Tensor rowptr, Tensor col, OptTensor opt_value,
                OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor mat) {
  return spmm_add(opt_row, rowptr, col, opt_value, std::nullopt, opt_colptr, opt_csr2csc, mat, false, false);
}

Tensor spmm_mean(OptTensor opt_row, Tensor rowptr, Tensor col, OptTensor opt_value,
                 OptTensor opt_rowcount, OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor mat) {
  return spmm_add(opt_row, rowptr, col, opt_value, opt_rowcount, opt_colptr, opt_csr2csc, mat, true, false);
}

Tensor spmm_sum_owned(OptTensor opt_row, Tensor rowptr, Tensor col, OptTensor opt_value,
                      OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor mat) {
  return spmm_add(opt_row, rowptr, col, opt_value, std::nullopt, opt_colptr, opt_csr2csc, mat, false, true);
}

Tensor spmm_mean_owned(OptTensor opt_row, Tensor rowptr, Tensor col, OptTensor opt_value,
                       OptTensor opt_rowcount, OptTensor opt_colptr, OptTensor opt_csr2csc, Tensor mat) {
  return spmm_add(opt_row, rowptr, col, opt_value, opt_rowcount, opt_colptr, opt_csr2csc, mat, true, true);
}

// tsamd::spmm_minmax(Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor? csr2csc, Tensor? row,
//                    Tensor mat, bool is_max, bool arg32) -> (Tensor, Tensor)
// spmm_min / spmm_max with the CSC arrays of the matrix: same forward, atomic-free deterministic backward.
// arg32: the second result holds the winners as int32 ids (for callers that only keep it for this backward:
// SparseTensor.matmul returns `out` alone) -- half the bytes written by the forward and read by the backward.
std::tuple<Tensor, Tensor> spmm_minmax(Tensor rowptr, Tensor col, OptTensor opt_value, OptTensor opt_colptr,
                                       OptTensor opt_csr2csc, OptTensor opt_row, Tensor mat, bool is_max, bool arg32) {
  auto r = SpmmMinMaxFunction::apply(rowptr, col, opt_value.value_or(col), mat, opt_value.has_value(), is_max,
                                     opt_colptr, opt_csr2csc, opt_row, arg32);
  return std::make_tuple(r[0], r[1]);
}

std::tuple<Tensor, Tensor> spmm_min(Tensor rowptr, Tensor col, OptTensor opt_value, Tensor mat) {
  return spmm_minmax(rowptr, col, opt_value, std::nullopt, std::nullopt, std::nullopt, mat, false, false);
}

std::tuple<Tensor, Tensor> spmm_max(Tensor rowptr, Tensor col, OptTensor opt_value, Tensor mat) {
  return spmm_minmax(rowptr, col, opt_value, std::nullopt, std::nullopt, std::nullopt, mat, true, false);
}

Tensor ind2ptr(Tensor ind, int64_t M) {
  check_gpu(ind, "ind");
  TORCH_CHECK(ind.scalar_type() == at::kLong, "ind must be int64");
  c10::hip::HIPGuard guard(ind.get_device());
  ind = ind.contiguous();
  Tensor out = torch::empty({M + 1}, ind.options());
  check_status(tsamd_ind2ptr(ind.data_ptr<int64_t>(), M, ind.numel(), out.data_ptr<int64_t>(),
                             current_stream(ind)),
               "tsamd_ind2ptr");
  return out;
}

Tensor ptr2ind(Tensor ptr, int64_t E) {
  check_gpu(ptr, "ptr");
  TORCH_CHECK(ptr.scalar_type() == at::kLong, "ptr must be int64");
  c10::hip::HIPGuard guard(ptr.get_device());
  ptr = ptr.contiguous();
  Tensor out = torch::empty({E}, ptr.options());
  check_status(tsamd_ptr2ind(ptr.data_ptr<int64_t>(), ptr.numel() - 1, E, out.data_ptr<int64_t>(),
                             current_stream(ptr)),
               "tsamd_ptr2ind");
  return out;
}

// torch_sparse.spmm(index, value, m, n, matrix) on a small unsorted COO: ONE launch (tsamd_spmm_coo_small).  No
// autograd: the Python front-end takes this route only when nothing asks for a gradient.
bool spmm_coo_small_supported(Tensor value, int64_t E, int64_t M, int64_t K) {
  switch (value.scalar_type()) {
    case at::kFloat: case at::kDouble: case at::kHalf: case at::kBFloat16: case at::kInt: case at::kLong:
    case at::kByte: case at::kChar: case at::kShort: break;
    default: return false;
  }
  return tsamd_spmm_coo_small_supported(dtype_code(value), E, M, K) != 0;
}

// -> the product [M, K], or an EMPTY 1-D tensor when the direct route does not take this problem (too big, a batch
// of matrices, a dtype it has no kernel for): one operator call decides and computes, the caller falls through to the
// sorted route on the sentinel.
Tensor spmm_coo_small(Tensor index, Tensor value, int64_t M, int64_t N, Tensor mat) {
  if (!(index.device().is_cuda() && value.device().is_cuda() && mat.device().is_cuda()) || mat.dim() != 2 ||
      index.dim() != 2 || index.size(0) != 2 || index.scalar_type() != at::kLong || value.dim() != 1 ||
      value.size(0) != index.size(1) || value.scalar_type() != mat.scalar_type() || mat.size(0) != N ||
      !spmm_coo_small_supported(value, index.size(1), M, mat.size(1)))
    return torch::empty({0}, mat.options().requires_grad(false));
  c10::hip::HIPGuard guard(mat.get_device());
  index = index.contiguous();
  value = value.contiguous();
  mat = mat.contiguous();
  const int64_t E = index.size(1), K = mat.size(1);
  Tensor out = torch::empty({M, K}, mat.options().requires_grad(false));
  check_status(tsamd_spmm_coo_small(dtype_code(mat), index.data_ptr<int64_t>(), index.data_ptr<int64_t>() + E,
                                    value.data_ptr(), mat.data_ptr(), out.data_ptr(), E, M, N, K, current_stream(mat)),
               "tsamd_spmm_coo_small");
  return out;
}

int64_t cuda_version() { return tsamd_hip_version(); }

// tsamd_spmm_reference_order (include/tsamd.h): 1 = every SpMM forward in the reference CPU kernel's order of
// operations (bit-identical results, slow), 0 = the product kernels, anything else = query; returns the mode in force
int64_t reference_order(int64_t set) { return (int64_t)tsamd_spmm_reference_order((int)set); }

// tsamd_spmm_column_order (include/tsamd.h): 0 = the merge kernel runs its partitions in their own order, 1 = auto,
// 2 = column order for every call in scope, anything else = query; returns the setting in force
int64_t column_order(int64_t set) { return (int64_t)tsamd_spmm_column_order((int)set); }

// torch.are_deterministic_algorithms_enabled() for TorchScript callers (storage_spmm)
bool deterministic_mode() { return at::globalContext().deterministicAlgorithms(); }


}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_spmm = torch::RegisterOperators()
                           .op("torch_sparse::spmm_sum", &spmm_sum)
                           .op("torch_sparse::spmm_mean", &spmm_mean)
                           .op("torch_sparse::spmm_min", &spmm_min)
                           .op("torch_sparse::spmm_max", &spmm_max)
                           .op("torch_sparse::ind2ptr", &ind2ptr)
                           .op("torch_sparse::ptr2ind", &ptr2ind)
                           .op("torch_sparse::cuda_version", &cuda_version)
                           .op("tsamd::spmm_coo_small", &spmm_coo_small)
                           .op("tsamd::spmm_coo_small_supported", &spmm_coo_small_supported)
                           .op("tsamd::spmm_minmax", &spmm_minmax)
                           .op("tsamd::deterministic", &deterministic_mode)
                           .op("tsamd::reference_order", &reference_order)
                           .op("tsamd::column_order", &column_order)
                           .op("tsamd::spmm_sum_owned", &spmm_sum_owned)
                           .op("tsamd::spmm_mean_owned", &spmm_mean_owned)
                           .op("tsamd::relabel_ids", &relabel_ids)
                           .op("tsamd::gather_rows", &gather_rows)
                           .op("tsamd::spmm_relabelled", &spmm_relabelled);
