// Dual report kernel (acn_qp_duals.hpp): instantiations and launcher.
#include "acn_qp_duals.hpp"

namespace acnqp {

hipError_t launch_duals(const DualsArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (duals_wave_shape(a.N, a.Tm)) {
    hipLaunchKernelGGL(duals_kernel<true>, dim3(a.B), dim3(64), duals_wave_lds(a.N, a.Tm), st, a);
  } else {
    // one thread per EVSE in the session phase (N <= 1024)
    const int threads = a.N <= 256 ? 256 : (a.N <= 512 ? 512 : 1024);
    hipLaunchKernelGGL(duals_kernel<false>, dim3(a.B), dim3(threads), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace acnqp
