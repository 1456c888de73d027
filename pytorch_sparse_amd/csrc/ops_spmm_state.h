// What the SpMM operator glue keeps between calls (ops_spmm_state.cpp): the operand cache, the transposed-pattern cache
// and the pattern hints.  ops_spmm.cpp asks through these calls only; entries, keys, locks, switches and the control
// operators (tsamd::operand_cache, pattern_cache, pattern_cache_stats, pattern_hints) are private to the unit.
#pragma once

#include "ops_common.h"

namespace tsamd_ops {

// No cache may hold on to memory that was allocated while a HIP graph is being captured (it would come from the
// graph's private pool): a capturing stream bypasses them.
bool stream_is_capturing(void *stream);

// ---- operand cache ------------------------------------------------------------------------------------------------
bool operand_cache_enabled();

// The buffer that tsamd_spmm_cached keeps the relabelled copy of `mat` in, for a product that needs `bytes` of it
// (tsamd_spmm_operand_cache_bytes != 0) on checked arguments.  buf undefined: the call goes without (cache off, an
// operand that cannot be remembered, a capturing stream).  valid: buf holds this operand's copy already.  `held` keeps
// the entry locked until the caller has enqueued the product that fills or reads buf: let it go out of scope after that.
struct OperandCopy {
  Tensor buf;
  bool valid = false;
  std::unique_lock<std::mutex> held;
};
OperandCopy operand_cache_copy(const Tensor &col, const Tensor &mat, int dt, int red, int64_t E, size_t bytes);

// ---- transposed-pattern cache -------------------------------------------------------------------------------------
// The CSC view of one backward, under one lock acquisition.  row_t: row[csr2csc] from the cache, or undefined when the
// caller should read through csr2csc instead (cache off, tensors that cannot be remembered, or the FIRST backward with
// this pattern).  value_t: value[csr2csc], only with a defined row_t and want_values -- kept across backwards when
// `value` is not trainable, gathered anew otherwise.
struct CscView {
  Tensor row_t, value_t;
};
CscView pattern_cache_csc_view(const Tensor &row, const Tensor &csr2csc, const OptTensor &value, bool want_values);

// ---- pattern hints ------------------------------------------------------------------------------------------------
// The hints buffer of this call's pattern and what to do with it (1 build, 2 reuse), or state 0: the call goes without.
// `like`: a tensor on the call's device (the buffer is allocated under the current stream).
std::pair<Tensor, int> pattern_hints_for(const Tensor &rowptr, const Tensor &col, int dt, int red, int64_t B, int64_t M,
                                         int64_t N, int64_t K, int64_t E, const Tensor &like, void *stream);
// a build call failed: its entry holds nothing a later call may reuse
void pattern_hints_drop(const Tensor &buf);

}  // namespace tsamd_ops
