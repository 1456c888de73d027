// torch operator glue, part 8: fused GATv2 attention (csrc/gatv2.hip) -- the forward, the entry kernel of the backward
// (p, ds) and the segment kernel that turns ds into the gradients of x_dst, x_src and att.  See ops_spmm.cpp for the conventions; pytorch_sparse_amd/attention.py holds the autograd function.
#include "ops_common.h"

namespace tsamd_ops {
namespace {

// x_dst [M, H, D], x_src [N, H, D], att [H, D] of one dtype on one device -> made contiguous
void check_gatv2(const Tensor &ptr, const Tensor &ind, Tensor &xa, Tensor &xb, Tensor &att, double negative_slope,
                 const char *na, const char *nb) {
  check_index(ptr, "ptr");
  check_index(ind, "ind");
  check_gpu(xa, na);
  check_gpu(xb, nb);
  check_gpu(att, "att");
  TORCH_CHECK(xa.dim() == 3 && xb.dim() == 3, na, " and ", nb, " must be [rows, heads, features], got ", xa.dim(),
              " and ", xb.dim(), " dimension(s)");
  TORCH_CHECK(att.dim() == 2, "att must be [heads, features], got ", att.dim(), " dimension(s)");
  TORCH_CHECK(xa.scalar_type() == at::kFloat || xa.scalar_type() == at::kBFloat16,
              "gatv2_attention: float32 or bfloat16 expected, got ", xa.scalar_type());
  TORCH_CHECK(xa.scalar_type() == xb.scalar_type() && xa.scalar_type() == att.scalar_type(), na, ", ", nb,
              " and att differ in dtype: ", xa.scalar_type(), ", ", xb.scalar_type(), " and ", att.scalar_type());
  TORCH_CHECK(xa.get_device() == xb.get_device() && xa.get_device() == att.get_device() &&
                  xa.get_device() == ind.get_device(),
              na, ", ", nb, ", att and the pattern must be on one device");
  TORCH_CHECK(xa.size(1) == xb.size(1) && xa.size(2) == xb.size(2), na, " is ", xa.sizes().slice(1), " per row, ", nb,
              " is ", xb.sizes().slice(1), ": heads and features must agree");
  TORCH_CHECK(att.size(0) == xa.size(1) && att.size(1) == xa.size(2), "att must be [", xa.size(1), ", ", xa.size(2),
              "], got ", att.sizes());
  TORCH_CHECK(ptr.numel() == xa.size(0) + 1, "ptr has ", ptr.numel(), " elements, ", na, " has ", xa.size(0), " rows");
  TORCH_CHECK(std::isfinite(negative_slope), "negative_slope must be finite, got ", negative_slope);
  xa = xa.contiguous();
  xb = xb.contiguous();
  att = att.contiguous();
}

// (out [M, H, D], lse [M, H] float, out_acc: out before its rounding as float where keep_acc asks for it and the dtype
// is not float32, else out itself)
std::tuple<Tensor, Tensor, Tensor> gatv2_attention_heads(Tensor rowptr, Tensor col, Tensor x_dst, Tensor x_src,
                                                         Tensor att, double negative_slope, bool keep_acc) {
  check_gatv2(rowptr, col, x_dst, x_src, att, negative_slope, "x_dst", "x_src");
  const int64_t M = x_dst.size(0), N = x_src.size(0), H = x_dst.size(1), D = x_dst.size(2), E = col.numel();
  TORCH_CHECK(D > 0 || M * H == 0, "gatv2_attention_heads needs at least one feature per head");
  c10::hip::HIPGuard guard(x_dst.get_device());
  rowptr = rowptr.contiguous();
  col = col.contiguous();
  Tensor out = torch::empty({M, H, D}, x_dst.options().requires_grad(false));
  Tensor lse = torch::empty({M, H}, x_dst.options().dtype(at::kFloat).requires_grad(false));
  const bool acc = keep_acc && x_dst.scalar_type() != at::kFloat;
  Tensor out_acc = acc ? torch::empty({M, H, D}, lse.options()) : out;
  if (out.numel() == 0) return std::make_tuple(out, lse, out_acc);
  const int dt = dtype_code(x_dst);
  Tensor ws = workspace(tsamd_gatv2_workspace_bytes(dt, H, D, E), x_dst);
  check_status(tsamd_gatv2_attention(dt, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), x_dst.data_ptr(),
                                     x_src.data_ptr(), att.data_ptr(), negative_slope, out.data_ptr(),
                                     acc ? out_acc.data_ptr<float>() : nullptr, lse.data_ptr(), M, N, H, D, E, ws.data_ptr(), (size_t)ws.numel(), current_stream(x_dst)),
               "tsamd_gatv2_attention");
  return std::make_tuple(out, lse, out_acc);
}

// (p, ds), both [E, H] float; out_acc is the forward's third result
std::tuple<Tensor, Tensor> gatv2_attention_heads_bw(OptTensor row, Tensor rowptr, Tensor col, Tensor x_dst,
                                                    Tensor x_src, Tensor att, Tensor out_acc, Tensor lse, Tensor grad_out,
                                                    double negative_slope) {
  check_gatv2(rowptr, col, x_dst, x_src, att, negative_slope, "x_dst", "x_src");
  if (row.has_value()) check_index(row.value(), "row");
  check_gpu(out_acc, "out_acc");
  check_gpu(lse, "lse");
  check_gpu(grad_out, "grad_out");
  const int64_t M = x_dst.size(0), N = x_src.size(0), H = x_dst.size(1), D = x_dst.size(2), E = col.numel();
  TORCH_CHECK(grad_out.sizes() == x_dst.sizes(), "grad_out must have the shape of x_dst, got ", grad_out.sizes());
  TORCH_CHECK(out_acc.sizes() == x_dst.sizes() && out_acc.scalar_type() == at::kFloat &&
                  out_acc.get_device() == x_dst.get_device(),
              "out_acc must be float with the shape of x_dst, got ", out_acc.sizes(), " of ", out_acc.scalar_type());
  TORCH_CHECK(grad_out.scalar_type() == x_dst.scalar_type(), "grad_out and x_dst differ in dtype: ",
              grad_out.scalar_type(), " and ", x_dst.scalar_type());
  TORCH_CHECK(lse.dim() == 2 && lse.size(0) == M && lse.size(1) == H && lse.scalar_type() == at::kFloat,
              "lse must be [rows, heads] of float, got ", lse.sizes(), " of ", lse.scalar_type());
  TORCH_CHECK(grad_out.get_device() == x_dst.get_device() && lse.get_device() == x_dst.get_device(),
              "lse, grad_out and x_dst must be on one device");
  TORCH_CHECK(!row.has_value() || row.value().numel() == E, "row and col differ in length");
  TORCH_CHECK(D > 0 || E == 0 || H == 0, "gatv2_attention_heads_bw needs at least one feature per head");
  c10::hip::HIPGuard guard(x_dst.get_device());
  out_acc = out_acc.contiguous();
  lse = lse.contiguous();
  grad_out = grad_out.contiguous();
  rowptr = rowptr.contiguous();
  col = col.contiguous();
  Tensor r = row.has_value() ? row.value().contiguous() : Tensor();
  const auto opt = x_dst.options().dtype(at::kFloat).requires_grad(false);
  Tensor p = torch::empty({E, H}, opt), ds = torch::empty({E, H}, opt);
  if (p.numel() == 0) return std::make_tuple(p, ds);
  check_status(tsamd_gatv2_attention_bw(dtype_code(x_dst), row.has_value() ? r.data_ptr<int64_t>() : nullptr,
                                        rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), x_dst.data_ptr(),
                                        x_src.data_ptr(), att.data_ptr(), out_acc.data_ptr<float>(), lse.data_ptr(),
                                        grad_out.data_ptr(), negative_slope, p.data_ptr<float>(), ds.data_ptr<float>(),
                                        M, N, H, D, E, current_stream(x_dst)),
               "tsamd_gatv2_attention_bw");
  return std::make_tuple(p, ds);
}

// the segment kernel: (out [nseg, H, D], grad_att [H, D] or an empty tensor).  p and g given: the VALUE call
std::tuple<Tensor, Tensor> gatv2_grad(Tensor ptr, Tensor ind, OptTensor perm, Tensor u, Tensor w, Tensor att,
                                      double negative_slope, Tensor ds, OptTensor p, OptTensor g, bool want_att) {
  check_gatv2(ptr, ind, u, w, att, negative_slope, "u", "w");
  if (perm.has_value()) check_index(perm.value(), "perm");
  check_gpu(ds, "ds");
  const int64_t S = u.size(0), N = w.size(0), H = u.size(1), D = u.size(2), E = ind.numel();
  const bool value = p.has_value() || g.has_value();
  TORCH_CHECK(p.has_value() == g.has_value(), "p and g come together");
  TORCH_CHECK(!(value && want_att), "gatv2_grad: the value term and grad_att are separate calls");
  TORCH_CHECK(!perm.has_value() || perm.value().numel() == E, "perm and ind differ in length");
  TORCH_CHECK(ds.dim() == 2 && ds.size(0) == E && ds.size(1) == H && ds.scalar_type() == at::kFloat &&
                  ds.get_device() == u.get_device(),
              "ds must be [nnz, heads] of float on the device of u, got ", ds.sizes(), " of ", ds.scalar_type());

  TORCH_CHECK(D > 0 || E == 0 || H == 0, "gatv2_grad needs at least one feature per head");
  Tensor pp, gg;
  if (value) {
    pp = p.value();
    gg = g.value();
    check_gpu(pp, "p");
    check_gpu(gg, "g");
    TORCH_CHECK(pp.sizes() == ds.sizes() && pp.scalar_type() == at::kFloat && pp.get_device() == u.get_device(),
                "p must be like ds, got ", pp.sizes(), " of ", pp.scalar_type());
    TORCH_CHECK(gg.sizes() == w.sizes() && gg.scalar_type() == w.scalar_type() && gg.get_device() == u.get_device(),
                "g must be like w, got ", gg.sizes(), " of ", gg.scalar_type());
    pp = pp.contiguous();
    gg = gg.contiguous();
  }
  c10::hip::HIPGuard guard(u.get_device());
  ptr = ptr.contiguous();
  ind = ind.contiguous();
  ds = ds.contiguous();
  Tensor pm = perm.has_value() ? perm.value().contiguous() : Tensor();
  Tensor out = torch::empty({S, H, D}, u.options().requires_grad(false));
  Tensor ga = want_att ? torch::empty({H, D}, u.options().requires_grad(false)) : Tensor();
  if (H * D == 0 || (S == 0 && !want_att)) return std::make_tuple(out, want_att ? ga : torch::empty({0}, u.options()));
  const int dt = dtype_code(u);
  Tensor ws = workspace(tsamd_gatv2_workspace_bytes(dt, H, D, E), u);
  check_status(tsamd_gatv2_grad(dt, (value ? 1 : 0) | (want_att ? 2 : 0), ptr.data_ptr<int64_t>(),
                                ind.data_ptr<int64_t>(), perm.has_value() ? pm.data_ptr<int64_t>() : nullptr,
                                u.data_ptr(), w.data_ptr(), att.data_ptr(), negative_slope, ds.data_ptr<float>(),
                                value ? pp.data_ptr<float>() : nullptr, value ? gg.data_ptr() : nullptr,
                                out.data_ptr(), want_att ? ga.data_ptr() : nullptr, S, N, H, D, E, ws.data_ptr(),
                                (size_t)ws.numel(), current_stream(u)),
               "tsamd_gatv2_grad");
  return std::make_tuple(out, want_att ? ga : torch::empty({0}, u.options()));
}

}  // namespace
}  // namespace tsamd_ops

using namespace tsamd_ops;

static auto registry_gatv2 =
    torch::RegisterOperators()
        .op("tsamd::gatv2_attention_heads(Tensor rowptr, Tensor col, Tensor x_dst, Tensor x_src, Tensor att, "
            "float negative_slope, bool keep_acc=False) -> (Tensor, Tensor, Tensor)",
            &gatv2_attention_heads)
        .op("tsamd::gatv2_attention_heads_bw(Tensor? row, Tensor rowptr, Tensor col, Tensor x_dst, Tensor x_src, "
            "Tensor att, Tensor out_acc, Tensor lse, Tensor grad_out, float negative_slope) -> (Tensor, Tensor)",
            &gatv2_attention_heads_bw)
        .op("tsamd::gatv2_grad(Tensor ptr, Tensor ind, Tensor? perm, Tensor u, Tensor w, Tensor att, "
            "float negative_slope, Tensor ds, Tensor? p, Tensor? g, bool want_att) -> (Tensor, Tensor)",
            &gatv2_grad);
