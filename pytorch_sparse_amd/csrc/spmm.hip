// CSR SpMM forward: the entry points of include/tsamd.h (all but tsamd_spmm_partial*, csrc/spmm_partial.hip) and the
// sum / mean instantiations of the kernels of spmm_kernels.h, which also says how the work is cut into units.
#define TSAMD_SPMM_PARTIAL_BUILD 0
#include "spmm_kernels.h"

#include <atomic>

using namespace tsamd;

// sum / mean are instantiated here, min / max in spmm_min.hip / spmm_max.hip
static int spmm_run(const SpmmCall &c) {
  return spmm_entry(c, [&](const SpmmPlan &p) -> int {
    if (c.reduce == TSAMD_MIN) return spmm_launch_min(c, p);
    if (c.reduce == TSAMD_MAX) return spmm_launch_max(c, p);
    return TSAMD_DISPATCH_DTYPE_ALL(c.dtype, [&]() -> int { return dispatch_spmm<scalar_t, RED_ADD>(c, p); });
  });
}

// The inspection entries (include/tsamd.h) plan the call they are asked about as the driver does and copy words out:
// plan_spmm's query mode.  `masked`: the call is spmm_masked_sum's (the pull of the min / max backward).
static SpmmPlan query_plan(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E, const void *mat,
                           const void *out, const void *arg_out, bool arg32, void *workspace, bool masked) {
  SpmmCall c{dtype, reduce, nullptr, nullptr, nullptr, mat, const_cast<void *>(out),
             reinterpret_cast<int64_t *>(const_cast<void *>(arg_out)), B, M, N, K, E, workspace, 0, nullptr};
  c.arg32 = arg32;
  if (masked) c.wmask = reinterpret_cast<const uint32_t *>(&c);  // present; never dereferenced
  return plan_spmm(c, true);
}

extern "C" size_t tsamd_spmm_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M,
                                             int64_t N, int64_t K, int64_t E) {
  if (dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  return carve(nullptr, dtype, reduce, B, M, N, K, E, nullptr);
}

extern "C" int tsamd_spmm(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                          const void *value, const void *mat, void *out, int64_t *arg_out,
                          int64_t B, int64_t M, int64_t N, int64_t K, int64_t E, void *workspace,
                          size_t workspace_bytes_given, void *stream_) {
  return spmm_run(SpmmCall{dtype, reduce, rowptr, col, value, mat, out, arg_out, B, M, N, K, E, workspace,
                           workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)});
}

// hot rows / hot blocks (include/tsamd.h), for callers that look into the workspace.  `blocks` says which of the two
// routes is asked about; a call takes at most one of them.
static int hot_layout(bool blocks, int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                      const void *mat, const void *out, void *workspace, int64_t *layout) {
  if (!layout || !workspace || !mat) return 0;
  const SpmmPlan p = query_plan(dtype, reduce, B, M, N, K, E, mat, out, nullptr, false, workspace, false);
  if (p.status != TSAMD_OK || p.what != SpmmPlan::Run || p.copy != (blocks ? 3 : 2)) return 0;
  const char *base = reinterpret_cast<const char *>(workspace);
  layout[0] = reinterpret_cast<const char *>(p.ws.hot_flag) - base;
  layout[1] = reinterpret_cast<const char *>(blocks ? p.ws.blk_word : p.ws.hot_word) - base;
  layout[2] = reinterpret_cast<const char *>(p.ws.hot_side) - base;
  layout[3] = p.ws.hot_side_row;
  return 1;
}

extern "C" int tsamd_spmm_hot_rows_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                          const void *mat, const void *out, void *workspace, int64_t *layout) {
  return hot_layout(false, dtype, reduce, B, M, N, K, E, mat, out, workspace, layout);
}

extern "C" int tsamd_spmm_hot_blocks_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                            const void *mat, const void *out, void *workspace, int64_t *layout) {
  return hot_layout(true, dtype, reduce, B, M, N, K, E, mat, out, workspace, layout);
}

extern "C" int tsamd_spmm_hot_block_min(void) { return kHotBlockMin; }

// column order (include/tsamd.h; spmm_kernels.h, section 1b): the process-wide setting, and where a call's order sits
namespace tsamd {
namespace {
std::atomic<int> g_column_order{1};
}
int spmm_column_order_mode() { return g_column_order.load(std::memory_order_relaxed); }
}  // namespace tsamd

extern "C" int tsamd_spmm_column_order(int set) {
  if (set >= 0 && set <= 2) tsamd::g_column_order.store(set, std::memory_order_relaxed);
  return tsamd::g_column_order.load(std::memory_order_relaxed);
}

extern "C" int tsamd_spmm_order_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                       const void *mat, const void *out, void *workspace, int64_t *layout) {
  if (!layout || !workspace) return 0;
  const SpmmPlan p = query_plan(dtype, reduce, B, M, N, K, E, mat, out, nullptr, false, workspace, false);
  if (p.status != TSAMD_OK || p.what != SpmmPlan::Run || p.order_mode == 0) return 0;
  const char *base = reinterpret_cast<const char *>(workspace);
  layout[0] = reinterpret_cast<const char *>(p.ws.order_hdr) - base;
  layout[1] = reinterpret_cast<const char *>(p.ws.order) - base;
  layout[2] = p.ws.P;
  layout[3] = reinterpret_cast<const char *>(p.ws.order_cls) - base;
  layout[4] = p.ws.order_shift;
  layout[5] = kOrderMinSingles;
  layout[6] = kOrderBucketMax;
  layout[7] = 0;
  return p.order_mode;
}

// The words of tsamd_spmm_route (include/tsamd.h) out of the call's plan.  Family: the merge instantiation, by the name of
// its shape -- the masked sum's is cooperative at every width, the record writers' are arg32_cooperative.
int tsamd::spmm_route_words(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E, const void *mat,
                            const void *out, const void *arg_out, int arg32, void *workspace, bool masked,
                            int64_t route[24]) {
  const SpmmPlan p = query_plan(dtype, reduce, B, M, N, K, E, mat, out, arg_out, arg32 != 0, workspace, masked);
  if (!route || p.status == TSAMD_ERR_INVALID) return TSAMD_ERR_INVALID;  // (a query's only INVALID: a negative size)
  for (int i = 0; i < 24; ++i) route[i] = 0;
  if (p.status != TSAMD_OK || p.what == SpmmPlan::Nothing) return p.status;  // family 0: nothing is launched
  if (p.what == SpmmPlan::ReferenceOrder) {
    route[0] = 7;
    return TSAMD_OK;
  }
  const Workspace &ws = p.ws;
  route[0] = p.merge == kMergeMasked ? kMergeCoop : (p.merge > kMergeMasked ? kMergeArg32Coop : p.merge);
  route[1] = p.vec;
  route[2] = p.lay.slots;
  route[3] = p.lay.lpr;
  route[4] = p.lay.lgG;
  route[5] = p.lay.ktiles;
  route[6] = ws.P;
  route[7] = ws.items;
  route[8] = ws.snap;
  route[9] = ws.relabel_mode;
  route[10] = p.copy;
  route[11] = p.fixup != kFixupNone ? 1 : 0;
  if (workspace) {
    const char *base = reinterpret_cast<const char *>(workspace);
    route[12] = reinterpret_cast<const char *>(ws.table) - base;
    route[13] = reinterpret_cast<const char *>(ws.tail_row) - base;
    route[14] = reinterpret_cast<const char *>(ws.head_row) - base;
    route[15] = reinterpret_cast<const char *>(ws.relabel_flag) - base;
  }
  route[16] = p.merge == kMergeRecords1 ? 1 : (p.merge == kMergeRecords2 ? 2 : 0);
  route[17] = B * (int64_t)p.lay.ktiles;
  route[18] = (int64_t)p.need;
  return TSAMD_OK;
}

extern "C" int tsamd_spmm_route(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                const void *mat, const void *out, const void *arg_out, int arg32, void *workspace,
                                int64_t route[24]) {
  return spmm_route_words(dtype, reduce, B, M, N, K, E, mat, out, arg_out, arg32, workspace, false, route);
}

// ---------------------------------------------------------------------------
// operand cache: see include/tsamd.h
// ---------------------------------------------------------------------------
extern "C" size_t tsamd_spmm_operand_cache_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N,
                                                 int64_t K, int64_t E) {
  (void)M;
  if (dtype_size(dtype) == 0 || B < 0 || N < 0 || K < 0 || E < 0) return 0;
  return operand_cache_bytes(dtype, reduce, B, N, K, E);
}

extern "C" size_t tsamd_spmm_cached_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N,
                                                    int64_t K, int64_t E) {
  if (dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  return carve(nullptr, dtype, reduce, B, M, N, K, E, nullptr, operand_cache_bytes(dtype, reduce, B, N, K, E) > 0);
}

extern "C" int tsamd_spmm_cached(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                                 const void *value, const void *mat, void *out, int64_t *arg_out, int64_t B,
                                 int64_t M, int64_t N, int64_t K, int64_t E, void *workspace,
                                 size_t workspace_bytes_given, void *cache, size_t cache_bytes, int cache_valid,
                                 void *stream_) {
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, arg_out, B, M, N, K, E, workspace,
             workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)};
  c.cache = cache;
  c.cache_bytes = cache_bytes;
  c.cache_valid = cache_valid;
  return spmm_run(c);
}

// ---------------------------------------------------------------------------
// pattern hints: see include/tsamd.h and spmm_kernels.h, section 1c
// ---------------------------------------------------------------------------
extern "C" size_t tsamd_spmm_hints_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E) {
  HintsLayout hl;
  return hints_layout(dtype, reduce, B, M, N, K, E, &hl) ? hl.bytes : 0;
}

extern "C" int tsamd_spmm_hints_layout(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                       int64_t *layout) {
  HintsLayout hl;
  if (!layout || !hints_layout(dtype, reduce, B, M, N, K, E, &hl)) return 0;
  layout[0] = (int64_t)hl.flags;
  layout[1] = (int64_t)hl.order_hdr;
  layout[2] = (int64_t)hl.blk_total;
  layout[3] = (int64_t)hl.blk_word;
  layout[4] = (int64_t)hl.blk_list;
  layout[5] = (int64_t)hl.order;
  layout[6] = hl.P;
  layout[7] = (int64_t)hl.bytes;
  return 1;
}

extern "C" int tsamd_spmm_hinted(int dtype, int reduce, const int64_t *rowptr, const int64_t *col, const void *value,
                                 const void *mat, void *out, int64_t *arg_out, int64_t B, int64_t M, int64_t N,
                                 int64_t K, int64_t E, void *workspace, size_t workspace_bytes_given, void *hints,
                                 int state, void *stream_) {
  if (!hints || (state != 1 && state != 2)) return TSAMD_ERR_INVALID;
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, arg_out, B, M, N, K, E, workspace,
             workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)};
  c.hints = hints;
  c.hints_state = state;
  return spmm_run(c);
}

// min / max with the winners as 32-bit entry ids (include/tsamd.h); cache == nullptr: stateless
extern "C" int tsamd_spmm_minmax_arg32(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                                       const void *value, const void *mat, void *out, int32_t *arg_out32, int64_t B,
                                       int64_t M, int64_t N, int64_t K, int64_t E, void *workspace,
                                       size_t workspace_bytes_given, void *cache, size_t cache_bytes, int cache_valid,
                                       void *stream_) {
  if (reduce != TSAMD_MIN && reduce != TSAMD_MAX) return TSAMD_ERR_UNSUPPORTED;
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, reinterpret_cast<int64_t *>(arg_out32), B, M, N, K,
             E, workspace, workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)};
  c.cache = cache;
  c.cache_bytes = cache_bytes;
  c.cache_valid = cache_valid;
  c.arg32 = true;
  return spmm_run(c);
}

// min / max whose forward leaves the winner RECORDS of the pull backward instead of the winner ids (include/tsamd.h).
// The merge kernel writes the records of the rows it finishes by itself (Workspace::rec_out) when the row shape allows
// it; the rows cut between partitions -- or every row, when it does not -- get theirs from the ids
// (minmax_winrec_kernel, csrc/spmm_bw.hip), which only live in the workspace.  spmm_emits_records (spmm_kernels.h) says which.
static size_t records_arg_bytes(int64_t B, int64_t M, int64_t K) { return align_up(sizeof(int32_t) * (size_t)(B * M * K), 256); }

extern "C" int tsamd_spmm_minmax_records_in_forward(int dtype, int64_t B, int64_t M, int64_t K, int64_t E) {
  return spmm_emits_records(dtype, B, M, K, E, nullptr, nullptr) ? 1 : 0;
}

extern "C" size_t tsamd_spmm_minmax_records_bytes(int64_t B, int64_t K, int64_t E) {
  if (B < 0 || K < 0 || E < 0) return 0;
  return align_up(sizeof(uint32_t) * (size_t)(B * E) * win_record_stride(K), 256);
}

// (the ids only exist -- in the workspace -- for the shapes whose records the forward does not write itself)
extern "C" size_t tsamd_spmm_minmax_records_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N,
                                                            int64_t K, int64_t E) {
  if (dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  return records_arg_bytes(B, M, K) + carve(nullptr, dtype, reduce, B, M, N, K, E, nullptr);
}

extern "C" int tsamd_spmm_minmax_records(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                                         const void *value, const void *mat, void *out, const int64_t *row,
                                         uint32_t *records, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                                         void *workspace, size_t workspace_bytes_given, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (reduce != TSAMD_MIN && reduce != TSAMD_MAX) return TSAMD_ERR_UNSUPPORTED;
  if (dtype != TSAMD_F32 && dtype != TSAMD_F64 && dtype != TSAMD_F16 && dtype != TSAMD_BF16) return TSAMD_ERR_UNSUPPORTED;
  if (B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return TSAMD_ERR_INVALID;
  if (E >= (int64_t)1 << 31 || M >= (int64_t)1 << 32) return TSAMD_ERR_UNSUPPORTED;
  if (B * M * K == 0) return TSAMD_OK;
  if (E > 0 && (!records || !row)) return TSAMD_ERR_INVALID;
  const size_t arg_b = records_arg_bytes(B, M, K);
  if (!workspace || workspace_bytes_given < tsamd_spmm_minmax_records_workspace_bytes(dtype, reduce, B, M, N, K, E) ||
      (uintptr_t)workspace % 256 != 0)
    return TSAMD_ERR_WORKSPACE;
  char *w = reinterpret_cast<char *>(workspace);
  int32_t *arg32 = reinterpret_cast<int32_t *>(w);
  void *inner = w + arg_b;
  const bool emit = E > 0 && spmm_emits_records(dtype, B, M, K, E, mat, out);
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, reinterpret_cast<int64_t *>(arg32), B, M, N, K, E,
             inner, workspace_bytes_given - arg_b, stream};
  c.arg32 = true;
  c.rec_out = emit ? records : nullptr;
  int st = spmm_run(c);
  if (st != TSAMD_OK || E == 0 || emit) return st;
  return minmax_winrec_from_ids(dtype, row, value, arg32, records, B, M, K, E, stream);
}

// ---------------------------------------------------------------------------
// relabelled ("camping-free") layout end to end: see include/tsamd.h
// ---------------------------------------------------------------------------
namespace tsamd {
namespace {
struct RelabelParams {
  uint32_t bits, mul, shift;
};
RelabelParams relabel_params(int64_t n) {
  RelabelParams p;
  p.bits = 1;
  while (p.bits < 32 && ((uint64_t)1 << p.bits) < (uint64_t)(n > 1 ? n : 2)) ++p.bits;
  p.mul = 0x9E3779B1u;
  p.shift = p.bits > 1 ? p.bits / 2 : 1;
  return p;
}
__global__ void relabel_ids_kernel(const int64_t *__restrict__ ids, int64_t count, uint32_t n,
                                   RelabelParams p, int64_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t v = ids ? ids[i] : i;
  out[i] = (v < 0 || v >= (int64_t)n) ? v : (int64_t)hash_row((uint32_t)v, n, p.bits, p.mul, p.shift);
}
}  // namespace
}  // namespace tsamd

// ---------------------------------------------------------------------------
// dst[i, :] = src[idx[i], :] for row-major matrices of `row_bytes`-byte rows: the pack step in front
// of a row exchange (pytorch_sparse_amd/parallel.py).  One packet (16 / 8 / 4 / 2 / 1 bytes, the
// widest the pitch and the pointers allow) per lane, 2^lgL lanes per row.
// ---------------------------------------------------------------------------
namespace tsamd {
namespace {
template <typename P>
__global__ __launch_bounds__(256) void gather_rows_kernel(const P *__restrict__ src,
                                                          const int64_t *__restrict__ idx,
                                                          P *__restrict__ dst, int64_t n, int64_t n_src,
                                                          uint32_t slots, int lgL) {
  const uint32_t lanes = 1u << lgL;
  const uint32_t sl0 = threadIdx.x & (lanes - 1);
  const int64_t rows_per_block = 256 >> lgL;
  for (int64_t r = (int64_t)blockIdx.x * rows_per_block + (threadIdx.x >> lgL); r < n;
       r += (int64_t)gridDim.x * rows_per_block) {
    int64_t j = idx[r];
    if (j < 0) j += n_src;  // torch indexing convention; the caller guarantees the range
    const P *s = src + (uint64_t)j * slots;
    P *d = dst + (uint64_t)r * slots;
    for (uint32_t sl = sl0; sl < slots; sl += lanes) d[sl] = s[sl];
  }
}

template <typename P>
int launch_gather_rows(const void *src, const int64_t *idx, void *dst, int64_t n, int64_t n_src,
                       int64_t row_bytes, hipStream_t stream) {
  const uint32_t slots = (uint32_t)(row_bytes / (int64_t)sizeof(P));
  int lgL = 0;
  while (lgL < 8 && (1u << lgL) < slots) ++lgL;
  const int64_t rows_per_block = 256 >> lgL;
  int64_t blocks = ceil_div(n, rows_per_block);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL((gather_rows_kernel<P>), dim3((unsigned int)blocks), dim3(256), 0, stream,
                     reinterpret_cast<const P *>(src), idx, reinterpret_cast<P *>(dst), n, n_src, slots, lgL);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}
}  // namespace
}  // namespace tsamd

extern "C" int tsamd_gather_rows(const void *src, const int64_t *idx, void *dst, int64_t n,
                                 int64_t n_src, int64_t row_bytes, void *stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (n < 0 || n_src < 0 || row_bytes < 0 || row_bytes >= (int64_t)1 << 32) return TSAMD_ERR_INVALID;
  if (n == 0 || row_bytes == 0) return TSAMD_OK;
  if (!src || !idx || !dst) return TSAMD_ERR_INVALID;
  const uintptr_t a = (uintptr_t)src | (uintptr_t)dst | (uintptr_t)row_bytes;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  if (a % 16 == 0) return launch_gather_rows<u32x4>(src, idx, dst, n, n_src, row_bytes, stream);
  if (a % 8 == 0) return launch_gather_rows<u32x2>(src, idx, dst, n, n_src, row_bytes, stream);
  if (a % 4 == 0) return launch_gather_rows<uint32_t>(src, idx, dst, n, n_src, row_bytes, stream);
  if (a % 2 == 0) return launch_gather_rows<uint16_t>(src, idx, dst, n, n_src, row_bytes, stream);
  return launch_gather_rows<uint8_t>(src, idx, dst, n, n_src, row_bytes, stream);
}

extern "C" int tsamd_relabel_ids(const int64_t *ids, int64_t count, int64_t n, int64_t *out,
                                 void *stream_) {
  if (count < 0 || n < 0 || n >= (int64_t)1 << 32) return TSAMD_ERR_UNSUPPORTED;
  if (count == 0) return TSAMD_OK;
  if (!out) return TSAMD_ERR_INVALID;
  hipLaunchKernelGGL(relabel_ids_kernel, dim3((unsigned int)ceil_div(count, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream_), ids, count, (uint32_t)n, relabel_params(n), out);
  TSAMD_LAUNCH_CHECK();
  return TSAMD_OK;
}

extern "C" size_t tsamd_spmm_relabelled_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M,
                                                        int64_t N, int64_t K, int64_t E) {
  if (dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  return carve(nullptr, dtype, reduce, B, M, N, K, E, nullptr, true);
}

extern "C" int tsamd_spmm_relabelled(int dtype, int reduce, const int64_t *rowptr,
                                     const int64_t *col_h, const void *value, const void *mat_h,
                                     void *out_h, int64_t *arg_out_h, int64_t B, int64_t M, int64_t N,
                                     int64_t K, int64_t E, void *workspace,
                                     size_t workspace_bytes_given, void *stream_) {
  SpmmCall c{dtype, reduce, rowptr, col_h, value, mat_h, out_h, arg_out_h, B, M, N, K, E, workspace,
             workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)};
  c.relabelled = true;
  return spmm_run(c);
}

extern "C" int tsamd_spmm_permuted(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                                   const void *value, const int64_t *perm, const void *mat, void *out,
                                   int64_t *arg_out, int64_t B, int64_t M, int64_t N, int64_t K,
                                   int64_t E, void *workspace, size_t workspace_bytes_given,
                                   void *stream_) {
  if (E > 0 && !perm) return TSAMD_ERR_INVALID;
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, arg_out, B, M, N, K, E, workspace,
             workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)};
  c.perm = perm;
  return spmm_run(c);
}

// internal (spmm_internal.h): the masked sum behind tsamd_spmm_minmax_bw_csc
namespace tsamd {
size_t spmm_masked_sum_workspace_bytes(int dtype, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E) {
  return carve(nullptr, dtype, TSAMD_SUM, B, M, N, K, E, nullptr, false, /*masked=*/true);
}
int spmm_masked_sum(int dtype, const int64_t *rowptr, bool has_value, const int64_t *perm,
                    const uint32_t *records, const void *mat, void *out, int64_t B, int64_t M, int64_t N,
                    int64_t K, int64_t E, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  if (E > 0 && !records) return TSAMD_ERR_INVALID;
  // `col` / `value` are only tested against NULL in the masked kernel (their contents come from the records)
  const int64_t *col = reinterpret_cast<const int64_t *>(records);
  const void *value = has_value ? reinterpret_cast<const void *>(records) : nullptr;
  SpmmCall c{dtype, TSAMD_SUM, rowptr, col, value, mat, out, /*arg_out=*/nullptr, B, M, N, K, E, workspace,
             workspace_bytes, stream};
  c.perm = perm;
  c.wmask = records;
  return spmm_run(c);
}
}  // namespace tsamd

extern "C" int tsamd_spmm_profiled(int dtype, int reduce, const int64_t *rowptr,
                                   const int64_t *col, const void *value, const void *mat,
                                   void *out, int64_t *arg_out, int64_t B, int64_t M, int64_t N,
                                   int64_t K, int64_t E, void *workspace,
                                   size_t workspace_bytes_given, void *stream_,
                                   float *kernel_ms_host) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  if (!kernel_ms_host) return TSAMD_ERR_INVALID;
  hipEvent_t ev[4];
  for (int i = 0; i < 4; ++i) TSAMD_HIP_TRY(hipEventCreate(&ev[i]));
  kernel_ms_host[0] = kernel_ms_host[1] = kernel_ms_host[2] = 0.f;
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, arg_out, B, M, N, K, E, workspace, workspace_bytes_given,
             stream};
  c.ev = ev;
  int st = spmm_run(c);
  if (st == TSAMD_OK && B * M * K > 0) {
    TSAMD_HIP_TRY(hipEventSynchronize(ev[3]));
    for (int i = 0; i < 3; ++i)
      TSAMD_HIP_TRY(hipEventElapsedTime(&kernel_ms_host[i], ev[i], ev[i + 1]));
  }
  for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
  return st;
}
