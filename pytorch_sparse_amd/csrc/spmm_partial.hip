// tsamd_spmm_partial: the SpMM kernels instantiated with the partial-product row sink (combine with what the earlier
// column blocks left in out / arg_out; include/tsamd.h).  A separate translation unit so that the instantiations behind
// every other entry point stay exactly as they were tuned -- and the two compile in parallel.
#define TSAMD_SPMM_PARTIAL_BUILD 1
#include "spmm_kernels.h"

using namespace tsamd;

extern "C" size_t tsamd_spmm_partial_workspace_bytes(int dtype, int reduce, int64_t B, int64_t M, int64_t N,
                                                     int64_t K, int64_t E) {
  if (dtype_size(dtype) == 0 || B < 0 || M < 0 || N < 0 || K < 0 || E < 0) return 0;
  return carve(nullptr, dtype, reduce, B, M, N, K, E, nullptr, true);
}

extern "C" int tsamd_spmm_partial(int dtype, int reduce, const int64_t *rowptr, const int64_t *col,
                                  const void *value, const void *mat, void *out, int64_t *arg_out, int64_t B,
                                  int64_t M, int64_t N, int64_t K, int64_t E, const int64_t *arg_map,
                                  int64_t arg_none, int accumulate, const int64_t *deg_rowptr, void *workspace,
                                  size_t workspace_bytes_given, void *stream_) {
  // E == 0 with accumulate: nothing to add; without: the "empty so far" state has to be written
  if (accumulate && E == 0 && reduce != TSAMD_MEAN) return TSAMD_OK;
  SpmmCall c{dtype, reduce, rowptr, col, value, mat, out, arg_out, B, M, N, K, E, workspace,
             workspace_bytes_given, reinterpret_cast<hipStream_t>(stream_)};
  c.partial = true;
  c.accumulate = accumulate;
  c.arg_map = arg_map;
  c.arg_none = arg_none;
  c.deg_rowptr = deg_rowptr;
  return spmm_entry(c, [&](const SpmmPlan &p) -> int {
    // partial products are the stages of the sharded SpMM over dense FEATURE matrices: floating point only
    if (dtype != TSAMD_F32 && dtype != TSAMD_F64 && dtype != TSAMD_F16 && dtype != TSAMD_BF16) return TSAMD_ERR_UNSUPPORTED;
    return TSAMD_DISPATCH_DTYPE_ALL(dtype, [&]() -> int {
      if constexpr (!(std::is_same<scalar_t, float>::value || std::is_same<scalar_t, double>::value ||
                      std::is_same<scalar_t, f16_t>::value || std::is_same<scalar_t, bf16_t>::value))
        return (int)TSAMD_ERR_UNSUPPORTED;
      else if (reduce == TSAMD_MIN)
        return dispatch_spmm<scalar_t, RED_MIN>(c, p);
      else if (reduce == TSAMD_MAX)
        return dispatch_spmm<scalar_t, RED_MAX>(c, p);
      else
        return dispatch_spmm<scalar_t, RED_ADD>(c, p);
    });
  });
}
