// The max instantiations of the SpMM kernels (and their int32-id variants); see the top of spmm_kernels.h.
#define TSAMD_SPMM_PARTIAL_BUILD 0
#include "spmm_kernels.h"

int tsamd::spmm_launch_max(int vec, const SpmmCall &c, const Workspace &ws) {
  return TSAMD_DISPATCH_DTYPE_ALL(c.dtype, [&]() -> int { return dispatch_spmm<scalar_t, RED_MAX>(vec, c, ws); });
}
