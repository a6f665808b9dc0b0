// Advance kernel (acn_qp_advance.hpp): instantiations and launcher.
#include "acn_qp_advance.hpp"

namespace acnqp {

hipError_t launch_advance(const AdvanceArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const size_t lds = advance_lds(a.N);
  const bool one = advance_threads(a.N) == 64;
  if (a.c_series) {   // rule 6b
    if (one) {
      hipLaunchKernelGGL((advance_kernel<64, true>), dim3(a.B), dim3(64), lds, st, a);
    } else {
      hipLaunchKernelGGL((advance_kernel<256, true>), dim3(a.B), dim3(256), lds, st, a);
    }
  } else if (one) {
    hipLaunchKernelGGL(advance_kernel<64>, dim3(a.B), dim3(64), lds, st, a);
  } else {
    hipLaunchKernelGGL(advance_kernel<256>, dim3(a.B), dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

}  // namespace acnqp
