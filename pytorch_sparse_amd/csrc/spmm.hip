// CSR SpMM forward: the entry points of include/tsamd.h (all but tsamd_spmm_partial*, csrc/spmm_partial.hip) and the
// sum / mean instantiations of the kernels of spmm_kernels.h, which also says how the work is cut into units.
#define TSAMD_SPMM_PARTIAL_BUILD 0
#include "spmm_kernels.h"

#include <atomic>

using namespace tsamd;

// sum / mean are instantiated here, min / max in spmm_min.hip / spmm_max.hip
static int spmm_run(const SpmmCall &c) {
  return spmm_entry(c, [&](int vec, const Workspace &ws) -> int {
    if (c.reduce == TSAMD_MIN) return spmm_launch_min(vec, c, ws);
    if (c.reduce == TSAMD_MAX) return spmm_launch_max(vec, c, ws);
    return TSAMD_DISPATCH_DTYPE_ALL(c.dtype, [&]() -> int { return dispatch_spmm<scalar_t, RED_ADD>(vec, c, ws); });
  });
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

// hot rows / hot blocks (include/tsamd.h): the host-side half of launch_spmm's decision, for callers that look into the
// workspace.  `blocks` says which of the two routes is asked about; a call takes at most one of them.
static int hot_layout(bool blocks, int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E,
                      const void *mat, const void *out, void *workspace, int64_t *layout) {
  if (!layout || !workspace || !mat || dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  if (dtype != TSAMD_F32 && dtype != TSAMD_F64 && dtype != TSAMD_F16 && dtype != TSAMD_BF16) return 0;
  if (spmm_reference_order_on() || (uintptr_t)workspace % 256 != 0) return 0;
  Workspace ws;
  carve(workspace, dtype, reduce, B, M, N, K, E, &ws);
  if ((ws.blk_word != nullptr) != blocks) return 0;
  const size_t es = dtype_size(dtype);
  const size_t packet = (es <= 2 ? 4 : 16 / es) * es;  // full-width packets (spmm_entry)
  if ((K * es) % packet != 0 || (uintptr_t)mat % packet != 0 || (uintptr_t)out % packet != 0) return 0;
  void *side = nullptr;
  int32_t side_row = 0;
  if (!hot_rows_place(ws, mat, blocks ? N + 64 : N, (uint64_t)K * es, &side, &side_row)) return 0;
  const char *base = reinterpret_cast<const char *>(workspace);
  layout[0] = reinterpret_cast<const char *>(ws.hot_flag) - base;
  layout[1] = reinterpret_cast<const char *>(blocks ? ws.blk_word : ws.hot_word) - base;
  layout[2] = reinterpret_cast<const char *>(side) - base;
  layout[3] = side_row;
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
  if (!layout || !workspace || dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  if (reduce != TSAMD_SUM && reduce != TSAMD_MEAN) return 0;
  if (B * M * K == 0 || spmm_reference_order_on() || (uintptr_t)workspace % 256 != 0) return 0;
  Workspace ws;
  carve(workspace, dtype, reduce, B, M, N, K, E, &ws);
  const int mode = order_mode_of(ws, dtype, reduce, N, K, E, lane_layout(K, packet_width(dtype, false, false, K, mat, out, nullptr)).lgG);
  if (mode == 0) return 0;
  const char *base = reinterpret_cast<const char *>(workspace);
  layout[0] = reinterpret_cast<const char *>(ws.order_hdr) - base;
  layout[1] = reinterpret_cast<const char *>(ws.order) - base;
  layout[2] = ws.P;
  layout[3] = reinterpret_cast<const char *>(ws.order_cls) - base;
  layout[4] = ws.order_shift;
  layout[5] = kOrderMinSingles;
  layout[6] = kOrderBucketMax;
  layout[7] = 0;
  return mode;
}

// min / max with int32 ids: which record-writing instantiation tsamd_spmm_minmax_records takes for these operands
// (0 = none: the records come from the ids)
static bool spmm_emits_records(int dtype, int64_t B, int64_t M, int64_t K, int64_t E, const void *mat, const void *out);

// What a forward call decides before it launches (include/tsamd.h): spmm_entry's checks in their order, then the
// planning functions of spmm_kernels.h and the instantiation chain of launch_spmm restated on the host.
// `masked`: the call is spmm_masked_sum's (the pull of the min / max backward) -- no reference-order mode, no probe of
// `col` (launch_spmm turns relabel mode 2 into 1 there) and hence no hot table.
int tsamd::spmm_route_words(int dtype, int reduce, int64_t B, int64_t M, int64_t N, int64_t K, int64_t E, const void *mat,
                            const void *out, const void *arg_out, int arg32, void *workspace, bool masked,
                            int64_t route[24]) {
  if (!route || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return TSAMD_ERR_INVALID;
  for (int i = 0; i < 24; ++i) route[i] = 0;
  if (reduce < TSAMD_SUM || reduce > TSAMD_MAX) return TSAMD_ERR_UNSUPPORTED;
  if (dtype_size(dtype) == 0) return TSAMD_ERR_UNSUPPORTED;
  if (N >= (int64_t)1 << 32 || K >= (int64_t)1 << 31 || B >= 65536) return TSAMD_ERR_UNSUPPORTED;
  if (B * ceil_div(K, 64) >= 65536) return TSAMD_ERR_UNSUPPORTED;
  const bool minmax = reduce == TSAMD_MIN || reduce == TSAMD_MAX;
  const bool floating = dtype == TSAMD_F32 || dtype == TSAMD_F64 || dtype == TSAMD_F16 || dtype == TSAMD_BF16;
  if (arg32 && !minmax) return TSAMD_ERR_UNSUPPORTED;  // (tsamd_spmm_minmax_arg32)
  if (B * M * K == 0) return TSAMD_OK;                 // family 0: nothing is launched
  if (spmm_reference_order_on() && !masked) {
    route[0] = 7;
    return TSAMD_OK;
  }
  if ((uintptr_t)workspace % 256 != 0) return TSAMD_ERR_WORKSPACE;
  if (arg32 && (E >= (int64_t)1 << 31 || !floating)) return TSAMD_ERR_UNSUPPORTED;
  // pointers count for their alignment and their distances only; without a workspace the layout is that of one that
  // starts at the first 256-byte boundary behind `mat`
  char *base = reinterpret_cast<char *>(workspace);
  if (!base) base = reinterpret_cast<char *>(align_up((size_t)(uintptr_t)mat + 1, 4096));
  if (!mat) mat = base;
  Workspace ws;
  route[18] = (int64_t)carve(base, dtype, reduce, B, M, N, K, E, &ws, false, masked);
  const int vec = packet_width(dtype, minmax, arg32 != 0, K, mat, out, arg_out);
  const LaneLayout lay = lane_layout(K, vec);
  const size_t es = dtype_size(dtype);
  const int max_vec = es <= 2 ? 4 : (int)(16 / es);
  int mode = ws.xperm != nullptr && vec > 1 ? 2 : 0;
  if (mode == 2 && masked) mode = 1;
  int copy = mode != 0 ? 1 : 0;
  if (mode == 2 && floating && !minmax && vec == max_vec && lay.lgG < 3) {  // kHotable, and launch_spmm's condition
    void *side = nullptr;
    int32_t side_row = 0;
    if (hot_rows_place(ws, mat, ws.blk_word != nullptr ? N + 64 : N, (uint64_t)K * es, &side, &side_row))
      copy = ws.blk_word != nullptr ? 3 : 2;
  }
  int family;
  if (arg32) family = lay.lgG >= 3 ? 5 : 6;
  else if (lay.lgG >= 3) family = 1;
  else family = copy == 2 ? 3 : (copy == 3 ? 4 : 2);
  route[0] = family;
  route[1] = vec;
  route[2] = lay.slots;
  route[3] = lay.lpr;
  route[4] = lay.lgG;
  route[5] = lay.ktiles;
  route[6] = ws.P;
  route[7] = ws.items;
  route[8] = minmax ? snap_items(ws.items) : 0;
  route[9] = mode;
  route[10] = copy;
  route[11] = ws.P > 1 ? 1 : 0;
  if (workspace) {
    route[12] = reinterpret_cast<char *>(ws.table) - base;
    route[13] = reinterpret_cast<char *>(ws.tail_row) - base;
    route[14] = reinterpret_cast<char *>(ws.head_row) - base;
    route[15] = reinterpret_cast<char *>(ws.relabel_flag) - base;
  }
  if (arg32 && E > 0 && vec == 4 && spmm_emits_records(dtype, B, M, K, E, mat, out))
    route[16] = ceil_div(K, 32) == 4 && win_record_stride(K) == 8u ? 1 : 2;
  route[17] = B * (int64_t)lay.ktiles;
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
// (minmax_winrec_kernel, csrc/spmm_bw.hip), which only live in the workspace.
static bool spmm_emits_records(int dtype, int64_t B, int64_t M, int64_t K, int64_t E, const void *mat, const void *out) {
  if (dtype != TSAMD_F32 && dtype != TSAMD_F16 && dtype != TSAMD_BF16) return false;
  if (K <= 32 || K > 256 || K % 4 != 0 || E >= (int64_t)1 << 31 || M >= (int64_t)1 << 32 || B < 1) return false;
  if (dtype == TSAMD_F32 && K <= 64) return false;  // measured even (profiles/r06_ab_fwd_winrec.md): the ids stay
  const size_t packet = 4 * dtype_size(dtype);  // the four-element packets the record writer's lane layout assumes
  if (mat != nullptr && (((uintptr_t)mat % packet) != 0 || ((uintptr_t)out % packet) != 0)) return false;
  return !spmm_reference_order_on();
}

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
