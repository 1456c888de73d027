// torch operator glue, part 7: sparse attention -- the multi-head SDDMM (csrc/sddmm.hip) and the multi-head SpMM over
// [nnz, H] values (csrc/spmm_heads.hip).  See ops_spmm.cpp for the conventions; pytorch_sparse_amd/attention.py holds
// the autograd pair.  (ptr, ind, perm) is a segmented order of the entries: (rowptr, col, None) or
// (colptr, row, csr2csc).
#include "ops_common.h"

namespace tsamd_ops {
namespace {

void check_heads_operand(const Tensor &t, const char *name) {
  check_gpu(t, name);
  TORCH_CHECK(t.dim() == 3, name, " must be [rows, heads, features], got ", t.dim(), " dimension(s)");
  TORCH_CHECK(at::isFloatingType(t.scalar_type()), name,
              ": float32, float64, float16 or bfloat16 expected, got ", t.scalar_type());
}

// scores[p(i), h] = scale * <q[s(i), h, :], k[ind[i], h, :]> -> [E, H] in storage order
Tensor sddmm_heads(OptTensor row, Tensor ptr, Tensor ind, OptTensor perm, Tensor q, Tensor k, double scale) {
  check_index(ptr, "ptr");
  check_index(ind, "ind");
  if (row.has_value()) check_index(row.value(), "row");
  if (perm.has_value()) check_index(perm.value(), "perm");
  check_heads_operand(q, "q");
  check_heads_operand(k, "k");
  TORCH_CHECK(q.scalar_type() == k.scalar_type(), "q and k differ in dtype: ", q.scalar_type(), " and ",
              k.scalar_type());
  TORCH_CHECK(q.get_device() == k.get_device() && q.get_device() == ind.get_device(),
              "q, k and the pattern must be on one device");
  TORCH_CHECK(q.size(1) == k.size(1), "q has ", q.size(1), " heads, k has ", k.size(1));
  TORCH_CHECK(q.size(2) == k.size(2), "q has ", q.size(2), " features per head, k has ", k.size(2));
  const int64_t nseg = q.size(0), nsrc = k.size(0), H = q.size(1), D = q.size(2), E = ind.numel();
  TORCH_CHECK(ptr.numel() == nseg + 1, "ptr has ", ptr.numel(), " elements, q has ", nseg, " rows");
  TORCH_CHECK(!row.has_value() || row.value().numel() == E, "row and ind differ in length");
  TORCH_CHECK(!perm.has_value() || perm.value().numel() == E, "perm and ind differ in length");
  c10::hip::HIPGuard guard(q.get_device());
  q = q.contiguous();
  k = k.contiguous();
  ptr = ptr.contiguous();
  ind = ind.contiguous();
  Tensor r = row.has_value() ? row.value().contiguous() : Tensor();
  Tensor p = perm.has_value() ? perm.value().contiguous() : Tensor();
  Tensor out = torch::empty({E, H}, q.options().requires_grad(false));
  if (E == 0 || H == 0) return out;
  if (D == 0) return out.zero_();  // an empty sum
  check_status(tsamd_sddmm_heads(dtype_code(q), row.has_value() ? r.data_ptr<int64_t>() : nullptr,
                                 ptr.data_ptr<int64_t>(), ind.data_ptr<int64_t>(),
                                 perm.has_value() ? p.data_ptr<int64_t>() : nullptr, q.data_ptr(), k.data_ptr(), scale,
                                 out.data_ptr(), nseg, nsrc, H, D, E, current_stream(q)),
               "tsamd_sddmm_heads");
  return out;
}

// out[s, h, :] = sum over the entries i of segment s of value[p(i), h] * x[ind[i], h, :] -> [nseg, H, D]
Tensor spmm_heads(Tensor ptr, Tensor ind, OptTensor perm, OptTensor value, Tensor x, int64_t nseg) {
  check_index(ptr, "ptr");
  check_index(ind, "ind");
  if (perm.has_value()) check_index(perm.value(), "perm");
  check_heads_operand(x, "x");
  TORCH_CHECK(x.get_device() == ind.get_device(), "x and the pattern must be on one device");
  const int64_t nsrc = x.size(0), H = x.size(1), D = x.size(2), E = ind.numel();
  TORCH_CHECK(nseg >= 0 && ptr.numel() == nseg + 1, "ptr has ", ptr.numel(), " elements for ", nseg, " segments");
  TORCH_CHECK(!perm.has_value() || perm.value().numel() == E, "perm and ind differ in length");
  c10::hip::HIPGuard guard(x.get_device());
  Tensor v;
  if (value.has_value()) {
    v = value.value();
    check_gpu(v, "value");
    TORCH_CHECK(v.dim() == 2, "value must be [nnz, heads], got ", v.dim(), " dimension(s)");
    TORCH_CHECK(v.size(0) == E, "value has ", v.size(0), " rows, the pattern has ", E, " entries");
    TORCH_CHECK(v.size(1) == H, "value has ", v.size(1), " heads, x has ", H);
    TORCH_CHECK(v.scalar_type() == x.scalar_type(), "value and x differ in dtype: ", v.scalar_type(), " and ",
                x.scalar_type());
    TORCH_CHECK(v.get_device() == x.get_device(), "value and x must be on one device");
    v = v.contiguous();
  }
  x = x.contiguous();
  ptr = ptr.contiguous();
  ind = ind.contiguous();
  Tensor p = perm.has_value() ? perm.value().contiguous() : Tensor();
  Tensor out = torch::empty({nseg, H, D}, x.options().requires_grad(false));
  if (out.numel() == 0) return out;
  const int dt = dtype_code(x);
  Tensor ws = workspace(tsamd_spmm_heads_workspace_bytes(dt, nseg, H, D, E), x);
  check_status(tsamd_spmm_heads(dt, ptr.data_ptr<int64_t>(), ind.data_ptr<int64_t>(),
                                perm.has_value() ? p.data_ptr<int64_t>() : nullptr,
                                value.has_value() ? v.data_ptr() : nullptr, x.data_ptr(), out.data_ptr(), nseg, nsrc, H,
                                D, E, ws.data_ptr(), (size_t)ws.numel(), current_stream(x)),
               "tsamd_spmm_heads");
  return out;
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_attention =
    torch::RegisterOperators()
        .op("tsamd::sddmm_heads(Tensor? row, Tensor ptr, Tensor ind, Tensor? perm, Tensor q, Tensor k, "
            "float scale=1.0) -> Tensor",
            &sddmm_heads)
        .op("tsamd::spmm_heads(Tensor ptr, Tensor ind, Tensor? perm, Tensor? value, Tensor x, int nseg) -> Tensor",
            &spmm_heads);
