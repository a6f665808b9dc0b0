// Adjoint of the advance kernel (acn_qp_advance_vjp.hpp): instantiations and launcher.
#include "acn_qp_advance_vjp.hpp"

namespace acnqp {

hipError_t launch_advance_vjp(const AdvanceVjpArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  const size_t lds = advance_vjp_lds(a.N);
  const bool one = advance_threads(a.N) == 64;   // the forward kernel's switch
  if (a.gprice && a.gq_next && a.c_weight) {     // A2
    if (one) {
      hipLaunchKernelGGL((advance_vjp_kernel<64, true>), dim3(a.B), dim3(64), lds, st, a);
    } else {
      hipLaunchKernelGGL((advance_vjp_kernel<256, true>), dim3(a.B), dim3(256), lds, st, a);
    }
  } else if (one) {
    hipLaunchKernelGGL(advance_vjp_kernel<64>, dim3(a.B), dim3(64), lds, st, a);
  } else {
    hipLaunchKernelGGL(advance_vjp_kernel<256>, dim3(a.B), dim3(256), lds, st, a);
  }
  return hipGetLastError();
}

}  // namespace acnqp
