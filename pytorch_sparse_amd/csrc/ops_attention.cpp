// torch operator glue, part 7: sparse attention -- the multi-head SDDMM (csrc/sddmm.hip) and the multi-head SpMM over
// [nnz, H] values (csrc/spmm_heads.hip), and the fused calls -- dot-product and additive (GAT) scores -- with their
// backward kernels (csrc/attention.hip).  See ops_spmm.cpp for the conventions; pytorch_sparse_amd/attention.py holds
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

// ---- the fused calls.  Dot-product and additive (GAT) scores differ in their operand checks, the names in the
// messages and the C entry points; below those the two score operands go by neutral names: sr belongs to the rows
// (q / a_dst), sc to the columns (k / a_src), the scalar is scale / negative_slope -------------------------------------
struct Fused {
  bool dot;
  const char *like_name;  // the operand the messages compare with: q (= sr) or v
  const char *fw, *bw;    // the C entry points; the operators carry these names without "tsamd_"
};
const Fused kDotScores = {true, "q", "tsamd_attention_heads", "tsamd_attention_heads_bw"};
const Fused kGatScores = {false, "v", "tsamd_gat_attention_heads", "tsamd_gat_attention_heads_bw"};
const char *op_name(const char *entry) { return entry + 6; }

// dropout on the probabilities: the rate and the seed of its mask (include/tsamd.h)
void check_dropout(double dropout, int64_t seed) {
  TORCH_CHECK(dropout >= 0.0 && dropout < 1.0, "dropout must be a rate in [0, 1), got ", dropout);
  TORCH_CHECK(seed >= 0, "seed must not be negative, got ", seed);
}

// the bias against the pattern and the operand `like` -> made contiguous (undefined without one)
Tensor check_bias(const OptTensor &bias, int64_t E, int64_t H, const Tensor &like, const char *like_name) {
  Tensor b;
  if (bias.has_value()) {
    b = bias.value();
    check_gpu(b, "bias");
    TORCH_CHECK(b.dim() == 1 || b.dim() == 2, "bias must be [nnz] or [nnz, heads], got ", b.dim(), " dimension(s)");
    TORCH_CHECK(b.size(0) == E, "bias has ", b.size(0), " rows, the pattern has ", E, " entries");
    TORCH_CHECK(b.dim() == 1 || b.size(1) == H, "bias has ", b.dim() == 2 ? b.size(1) : 1, " heads, ", like_name,
                " has ", H);
    TORCH_CHECK(b.scalar_type() == like.scalar_type(), "bias and ", like_name, " differ in dtype: ", b.scalar_type(),
                " and ", like.scalar_type());
    TORCH_CHECK(b.get_device() == like.get_device(), "bias and ", like_name, " must be on one device");
    b = b.contiguous();
  }
  return b;
}

// the checks both dot-product operators share -> the bias
Tensor check_attention(const Tensor &rowptr, const Tensor &col, const OptTensor &bias, const Tensor &q,
                       const Tensor &k, const Tensor &v) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  check_heads_operand(q, "q");
  check_heads_operand(k, "k");
  check_heads_operand(v, "v");
  TORCH_CHECK(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type(),
              "q, k and v differ in dtype: ", q.scalar_type(), ", ", k.scalar_type(), " and ", v.scalar_type());
  TORCH_CHECK(q.get_device() == k.get_device() && q.get_device() == v.get_device() &&
                  q.get_device() == col.get_device(),
              "q, k, v and the pattern must be on one device");
  TORCH_CHECK(q.size(1) == k.size(1), "q has ", q.size(1), " heads, k has ", k.size(1));
  TORCH_CHECK(q.size(2) == k.size(2), "q has ", q.size(2), " features per head, k has ", k.size(2));
  TORCH_CHECK(v.sizes() == k.sizes(), "v must have the shape of k, got ", v.sizes(), " and ", k.sizes());
  TORCH_CHECK(rowptr.numel() == q.size(0) + 1, "rowptr has ", rowptr.numel(), " elements, q has ", q.size(0),
              " rows");
  return check_bias(bias, col.numel(), q.size(1), q, "q");
}

// the checks both additive operators share -> the bias
Tensor check_gat_attention(const Tensor &rowptr, const Tensor &col, const OptTensor &bias, const Tensor &a_dst,
                           const Tensor &a_src, const Tensor &v, double negative_slope) {
  check_index(rowptr, "rowptr");
  check_index(col, "col");
  check_gpu(a_dst, "a_dst");
  check_gpu(a_src, "a_src");
  check_heads_operand(v, "v");
  TORCH_CHECK(a_dst.dim() == 2, "a_dst must be [rows, heads], got ", a_dst.dim(), " dimension(s)");
  TORCH_CHECK(a_src.dim() == 2, "a_src must be [columns, heads], got ", a_src.dim(), " dimension(s)");
  TORCH_CHECK(a_dst.scalar_type() == v.scalar_type() && a_src.scalar_type() == v.scalar_type(),
              "a_dst, a_src and v differ in dtype: ", a_dst.scalar_type(), ", ", a_src.scalar_type(), " and ",
              v.scalar_type());
  TORCH_CHECK(a_dst.get_device() == v.get_device() && a_src.get_device() == v.get_device() &&
                  v.get_device() == col.get_device(),
              "a_dst, a_src, v and the pattern must be on one device");
  TORCH_CHECK(a_dst.size(1) == v.size(1), "a_dst has ", a_dst.size(1), " heads, v has ", v.size(1));
  TORCH_CHECK(a_src.size(1) == v.size(1), "a_src has ", a_src.size(1), " heads, v has ", v.size(1));
  TORCH_CHECK(a_src.size(0) == v.size(0), "a_src has ", a_src.size(0), " rows, v has ", v.size(0));
  TORCH_CHECK(rowptr.numel() == a_dst.size(0) + 1, "rowptr has ", rowptr.numel(), " elements, a_dst has ",
              a_dst.size(0), " rows");
  TORCH_CHECK(std::isfinite(negative_slope), "negative_slope must be finite, got ", negative_slope);
  return check_bias(bias, col.numel(), v.size(1), v, "v");
}

// fused scores -> softmax over the row -> aggregation (csrc/attention.hip) -> (out [M, H, D], lse [M, H]); the operands
// have passed their checker, b is its bias.  The *_dropout entries serve every call: a rate of 0 is the plain call
std::tuple<Tensor, Tensor> fused_forward(const Fused &m, Tensor rowptr, Tensor col, const Tensor &b, Tensor sr,
                                         Tensor sc, Tensor v, double scalar, double dropout, int64_t seed) {
  check_dropout(dropout, seed);
  const int64_t M = sr.size(0), N = v.size(0), H = v.size(1), D = v.size(2), E = col.numel();
  c10::hip::HIPGuard guard(v.get_device());
  sr = sr.contiguous();
  sc = sc.contiguous();
  v = v.contiguous();
  rowptr = rowptr.contiguous();
  col = col.contiguous();
  Tensor out = torch::empty({M, H, D}, v.options().requires_grad(false));
  const auto acc = v.scalar_type() == at::kDouble ? at::kDouble : at::kFloat;
  Tensor lse = torch::empty({M, H}, v.options().dtype(acc).requires_grad(false));
  if (out.numel() == 0) {  // D == 0: every score would be its bias alone, nothing is aggregated
    TORCH_CHECK(D > 0 || lse.numel() == 0, op_name(m.fw), " needs at least one feature per head");
    return std::make_tuple(out, lse);
  }
  const int dt = dtype_code(v);
  Tensor ws = workspace(tsamd_attention_heads_workspace_bytes(dt, H, D, E), v);
  const auto call = m.dot ? tsamd_attention_heads_dropout : tsamd_gat_attention_heads_dropout;
  check_status(call(dt, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(), b.defined() ? b.data_ptr() : nullptr,
                    b.defined() && b.dim() == 2 ? H : 1, sr.data_ptr(), sc.data_ptr(), v.data_ptr(), scalar, dropout,
                    (uint64_t)seed, out.data_ptr(), lse.data_ptr(), M, N, H, D, E, ws.data_ptr(), (size_t)ws.numel(),
                    current_stream(v)),
               m.fw);
  return std::make_tuple(out, lse);
}

// p = e(s - lse[row]) and ds = p * (<grad_out[row], v[col]> - <grad_out[row], out[row]>), for the additive scores
// dz = ds * (z > 0 ? 1 : negative_slope) in its place -> two [E, H] arrays.  With dropout: pt = p * keep * c and
// ds = p * (keep * c * <grad_out[row], v[col]> - <grad_out[row], out[row]>)
std::tuple<Tensor, Tensor> fused_backward(const Fused &m, const OptTensor &row, Tensor rowptr, Tensor col,
                                          const Tensor &b, Tensor sr, Tensor sc, Tensor v, Tensor out, Tensor lse,
                                          Tensor grad_out, double scalar, double dropout, int64_t seed) {
  check_dropout(dropout, seed);
  if (row.has_value()) check_index(row.value(), "row");
  check_heads_operand(out, "out");
  check_heads_operand(grad_out, "grad_out");
  check_gpu(lse, "lse");
  const int64_t M = sr.size(0), N = v.size(0), H = v.size(1), D = v.size(2), E = col.numel();
  const Tensor &like = m.dot ? sr : v;
  if (m.dot) {
    TORCH_CHECK(out.sizes() == sr.sizes(), "out must have the shape of q, got ", out.sizes(), " and ", sr.sizes());
    TORCH_CHECK(grad_out.sizes() == sr.sizes(), "grad_out must have the shape of q, got ", grad_out.sizes(), " and ",
                sr.sizes());
  } else {
    TORCH_CHECK(out.dim() == 3 && out.size(0) == M && out.size(1) == H && out.size(2) == D,
                "out must be [rows, heads, features] = [", M, ", ", H, ", ", D, "], got ", out.sizes());
    TORCH_CHECK(grad_out.sizes() == out.sizes(), "grad_out must have the shape of out, got ", grad_out.sizes(),
                " and ", out.sizes());
  }
  TORCH_CHECK(out.scalar_type() == like.scalar_type() && grad_out.scalar_type() == like.scalar_type(),
              "out, grad_out and ", m.like_name, " differ in dtype: ", out.scalar_type(), ", ", grad_out.scalar_type(),
              " and ", like.scalar_type());
  const auto acc = like.scalar_type() == at::kDouble ? at::kDouble : at::kFloat;
  TORCH_CHECK(lse.dim() == 2 && lse.size(0) == M && lse.size(1) == H && lse.scalar_type() == acc,
              "lse must be [rows, heads] of ", acc, ", got ", lse.sizes(), " of ", lse.scalar_type());
  TORCH_CHECK(out.get_device() == like.get_device() && grad_out.get_device() == like.get_device() &&
                  lse.get_device() == like.get_device(),
              "out, lse, grad_out and ", m.like_name, " must be on one device");
  TORCH_CHECK(!row.has_value() || row.value().numel() == E, "row and col differ in length");
  TORCH_CHECK(D > 0 || E == 0 || H == 0, op_name(m.bw), " needs at least one feature per head");
  c10::hip::HIPGuard guard(v.get_device());
  sr = sr.contiguous();
  sc = sc.contiguous();
  v = v.contiguous();
  out = out.contiguous();
  lse = lse.contiguous();
  grad_out = grad_out.contiguous();
  rowptr = rowptr.contiguous();
  col = col.contiguous();
  Tensor r = row.has_value() ? row.value().contiguous() : Tensor();
  Tensor p = torch::empty({E, H}, v.options().requires_grad(false));
  Tensor d = torch::empty({E, H}, v.options().requires_grad(false));
  if (p.numel() == 0) return std::make_tuple(p, d);
  const auto call = m.dot ? tsamd_attention_heads_dropout_bw : tsamd_gat_attention_heads_dropout_bw;
  check_status(call(dtype_code(v), row.has_value() ? r.data_ptr<int64_t>() : nullptr, rowptr.data_ptr<int64_t>(),
                    col.data_ptr<int64_t>(), b.defined() ? b.data_ptr() : nullptr, b.defined() && b.dim() == 2 ? H : 1,
                    sr.data_ptr(), sc.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), grad_out.data_ptr(),
                    scalar, dropout, (uint64_t)seed, p.data_ptr(), d.data_ptr(), M, N, H, D, E, current_stream(v)),
               m.bw);
  return std::make_tuple(p, d);
}

std::tuple<Tensor, Tensor> attention_heads(Tensor rowptr, Tensor col, OptTensor bias, Tensor q, Tensor k, Tensor v,
                                           double scale, double dropout, int64_t seed) {
  Tensor b = check_attention(rowptr, col, bias, q, k, v);
  return fused_forward(kDotScores, rowptr, col, b, q, k, v, scale, dropout, seed);
}

std::tuple<Tensor, Tensor> attention_heads_bw(OptTensor row, Tensor rowptr, Tensor col, OptTensor bias, Tensor q,
                                              Tensor k, Tensor v, Tensor out, Tensor lse, Tensor grad_out,
                                              double scale, double dropout, int64_t seed) {
  Tensor b = check_attention(rowptr, col, bias, q, k, v);
  return fused_backward(kDotScores, row, rowptr, col, b, q, k, v, out, lse, grad_out, scale, dropout, seed);
}

std::tuple<Tensor, Tensor> gat_attention_heads(Tensor rowptr, Tensor col, OptTensor bias, Tensor a_dst, Tensor a_src,
                                               Tensor v, double negative_slope, double dropout, int64_t seed) {
  Tensor b = check_gat_attention(rowptr, col, bias, a_dst, a_src, v, negative_slope);
  return fused_forward(kGatScores, rowptr, col, b, a_dst, a_src, v, negative_slope, dropout, seed);
}

std::tuple<Tensor, Tensor> gat_attention_heads_bw(OptTensor row, Tensor rowptr, Tensor col, OptTensor bias,
                                                  Tensor a_dst, Tensor a_src, Tensor v, Tensor out, Tensor lse,
                                                  Tensor grad_out, double negative_slope, double dropout,
                                                  int64_t seed) {
  Tensor b = check_gat_attention(rowptr, col, bias, a_dst, a_src, v, negative_slope);
  return fused_backward(kGatScores, row, rowptr, col, b, a_dst, a_src, v, out, lse, grad_out, negative_slope, dropout,
                        seed);
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
            &spmm_heads)
        .op("tsamd::attention_heads(Tensor rowptr, Tensor col, Tensor? bias, Tensor q, Tensor k, Tensor v, "
            "float scale, float dropout=0.0, int seed=0) -> (Tensor, Tensor)",
            &attention_heads)
        .op("tsamd::attention_heads_bw(Tensor? row, Tensor rowptr, Tensor col, Tensor? bias, Tensor q, Tensor k, "
            "Tensor v, Tensor out, Tensor lse, Tensor grad_out, float scale, float dropout=0.0, int seed=0) -> "
            "(Tensor, Tensor)",
            &attention_heads_bw)
        .op("tsamd::gat_attention_heads(Tensor rowptr, Tensor col, Tensor? bias, Tensor a_dst, Tensor a_src, Tensor v, "
            "float negative_slope, float dropout=0.0, int seed=0) -> (Tensor, Tensor)",
            &gat_attention_heads)
        .op("tsamd::gat_attention_heads_bw(Tensor? row, Tensor rowptr, Tensor col, Tensor? bias, Tensor a_dst, "
            "Tensor a_src, Tensor v, Tensor out, Tensor lse, Tensor grad_out, float negative_slope, float dropout=0.0, "
            "int seed=0) -> (Tensor, Tensor)",
            &gat_attention_heads_bw);
