#pragma once
#include "common.h"
namespace tsamd {
// Stable sort of COO entries by (row, col) -- the order of row * N + col -- see sort.hip.  One call descriptor
// (SortCall) and one host driver (sort_coo_run) behind every entry point of the sort and of sort + coalesce.
// Inputs are not modified; outputs must not alias them.  E < 2^32, bits(M) + bits(N) <= 64.
// Ranking used by the radix kernels: 0 = one returning LDS atomic per entry (stable when the LDS unit serves the lanes
// of one instruction in ascending order -- checked on the device by a self-test the first time this is called),
// 1 = ballot matching (independent of that order).  sort_set_rank_mode(-1) forgets the decision (the next sort runs the
// self-test again), 0 / 1 force a mode (tests).
int sort_rank_mode(hipStream_t stream);
void sort_set_rank_mode(int mode);
size_t sort_coo_workspace_bytes(int64_t E);
bool sort_coo_supported(int64_t E, int64_t M, int64_t N);
// co (nullable): a COMPACTING sort.  When the bucket path sorts the input, its last kernel writes the distinct pairs
//   to co->row_u / col_u, the start of every run of equal pairs in the sorted order to co->seg_ptr (seg_ptr[nnz] = E)
//   and their number to co->nnz_out, and row_out / col_out / perm_out stay untouched; otherwise the one-sweep passes
//   write row_out / col_out (/ perm_out, nullable) as usual and the CALLER compacts them (it can tell on the device:
//   *sort_fast_flag(workspace, E) != 0 means the compacted outputs are already there).  co->status: nb words of scratch.
//   The one-launch sort (kSortSmall) compacts nothing, zeroes nothing and uses co->seg_ptr as its permutation.
//   Fused reduction (round 6): with a riding 4-byte value (SortCall::bytes == 4) and co->reduce >= 0 the bucket path also
//   REDUCES the values of every run -- sequentially in sorted order, in the accumulator type of
//   segment_reduce_kernel, i.e. the same bits -- into co->value_u (capacity E, entry p = the p-th distinct pair),
//   writes neither seg_ptr nor the sorted values, and sets *co->fused_out = 1 (the caller zeroes it beforehand).
struct SortCoalesce {
  int64_t *row_u, *col_u, *seg_ptr, *nnz_out;
  unsigned long long *status;  // [kSortCoalesceStatusWords]
  void *value_u = nullptr;     // [E] 4-byte elements, or null
  int64_t *fused_out = nullptr;
  int reduce = -1;             // -1: no fused reduction; 0 sum, 1 mean, 2 min, 3 max (TSAMD_SUM .. TSAMD_MAX)
  int is_float = 1;            // 4-byte value type: 1 float32, 0 int32
  bool no_seg = false;         // index only (no value to reduce afterwards): the bucket route does not write seg_ptr
  // the caller's zero-initialised state (the status words above, the state of its compaction kernel) lies in the
  // pre_zero_bytes bytes directly IN FRONT of `workspace`: the sort's first fill covers them too (one fill kernel
  // instead of three, ~4.5 us each); 0 = the sort zeroes co->status itself
  size_t pre_zero_bytes = 0;
};
constexpr int kSortCoalesceStatusWords = 1 << 14;
const unsigned long long *sort_fast_flag(void *workspace, int64_t E);
// {byte offset of the header in the sort's workspace, word index of #descents, of the fast word, of the error word}
// (tsamd_sort_header, coalesce.hip, adds what lies in front of the sort's workspace in a compacting call)
void sort_header_words(int64_t E, int64_t out[4]);
// Untrusted ids: every kernel behind sort_coo_run stays inside its buffers for ANY 64-bit row / col (the constructor
// enqueues the sort before its range check is read back).  sort_build_kernel keeps an id beyond its bit width out of
// the bucket histogram and bucket_plan_kernel then leaves the fast word at 0: such an input is sorted by the one-sweep
// passes, whose positions come from masked digits and ranks alone (sort.hip, UNTRUSTED IDS).  Its outputs mean nothing
// but lie inside their arrays, perm_out is a permutation, a riding value is value[perm_out], and counts[2..3] of a
// range-checking probe are the unsigned maxima.

// What decides whether the input is ordered at all -- on the device, without a host sync:
enum class SortOrder {
  kAlways,  // sort
  kProbe,   // the sort's first read of the input counts descents / adjacent duplicates into counts[0..1] (device), and
            // with 0 descents every later kernel returns at once: the outputs are a copy + the identity
  kProbed,  // the same, decided by counts[0] (device) of an earlier probe (tsamd_coo_check); nothing is written to it
};
// The route the driver took (tsamd_sort_route reports the same numbers from the sizes alone).
enum SortRoute {
  kSortIdentity = 0,  // nothing to order: at most one entry, or keys of zero bits
  kSortSmall = 1,     // the one-launch sort in LDS (plus a gather of the value through the permutation)
  kSortGeneral = 2,   // build + bucket path / one-sweep passes; which of the two sorted is decided on the device
};
struct SortCall {
  // input and outputs: row_out / col_out (nullable) the sorted ids, perm_out the position of every sorted entry in
  // the input (nullable only for a compacting sort)
  const int64_t *row, *col;
  int64_t E, M, N;
  int64_t *row_out, *col_out, *perm_out;
  SortOrder order = SortOrder::kAlways;
  int64_t *counts = nullptr;  // device; kProbe: written, kProbed: [0] read, kAlways: null
  // kProbe only: the probe also takes the maxima of the ids (as unsigned numbers) into counts[2..3] -- the range
  // check of the constructor.  Where it cannot ride in the build pass the driver launches tsamd_coo_check itself.
  bool range_check = false;
  // the riding value (both or neither): dst[o] = src[perm_out[o]] for arrays of 4- or 8-byte elements, written by
  // the sort's last kernel instead of a gather through perm_out later
  const void *src = nullptr;
  void *dst = nullptr;
  int64_t bytes = 0;
  const SortCoalesce *co = nullptr;  // a compacting sort, see above
  void *workspace = nullptr;         // sort_coo_workspace_bytes(E)
  size_t workspace_bytes = 0;
  // true: no workspace is asked for where the one-launch sort applies.  Kept for the C-ABI only: tsamd_sort_coo_auto /
  // _probed have always accepted a missing workspace there, every other entry point refuses it at any size.
  bool workspace_optional = false;
  hipStream_t stream = nullptr;
};
// Validates (TSAMD_ERR_INVALID / _UNSUPPORTED / _WORKSPACE as the entry points of include/tsamd.h document), picks
// the route and enqueues every launch of it; E == 0 is TSAMD_OK (kProbe: counts zeroed).  route_out (nullable): the
// route taken, written whenever something was launched.
int sort_coo_run(const SortCall &c, SortRoute *route_out = nullptr);
}  // namespace tsamd
