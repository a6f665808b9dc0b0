// Estimator kernel (acn_qp_estimate.hpp): instantiations and launcher.
#include "acn_qp_estimate.hpp"

namespace acnqp {

hipError_t launch_estimate(const EstimateArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const size_t lds = estimate_lds_bytes(a.N);   // (N <= 1024: at most 12 KiB)
  if (estimate_threads(a.N) == 64) {
    hipLaunchKernelGGL(estimate_kernel<64>, dim3(a.B), dim3(64), lds, st, a);
  } else {
    hipLaunchKernelGGL(estimate_kernel<256>, dim3(a.B), dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

}  // namespace acnqp
