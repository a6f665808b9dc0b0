// Select and hold kernels (acn_qp_hold.hpp): instantiations and launchers.
#include "acn_qp_hold.hpp"

namespace acnqp {

hipError_t launch_select(const SelectArgs& a, hipStream_t st) {
  if (a.m <= 0) return hipSuccess;
  if (hold_threads(a.N) == 64) {
    hipLaunchKernelGGL(select_kernel<64>, dim3(a.m), dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL(select_kernel<256>, dim3(a.m), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch_hold(const HoldArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (hold_threads(a.N) == 64) {
    hipLaunchKernelGGL(hold_kernel<64>, dim3(a.B), dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL(hold_kernel<256>, dim3(a.B), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace acnqp
