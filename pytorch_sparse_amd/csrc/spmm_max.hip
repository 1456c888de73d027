// The max instantiations of the SpMM kernels (and their int32-id variants); see the top of spmm_kernels.h.
#define TSAMD_SPMM_PARTIAL_BUILD 0
#include "spmm_kernels.h"

int tsamd::spmm_launch_max(const SpmmCall &c, const SpmmPlan &p) {
  return TSAMD_DISPATCH_DTYPE_ALL(c.dtype, [&]() -> int { return dispatch_spmm<scalar_t, RED_MAX>(c, p); });
}
