// Prepare kernel (acn_qp_prepare.hpp): instantiations and launcher.
#include "acn_qp_prepare.hpp"

namespace acnqp {

hipError_t launch_prepare(const PrepareArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  PrepareArgs k = a;
  const PrepareLayout lay = prepare_layout(a.N, a.M);
  k.site_lds = lay.site_lds;
  if (prepare_threads(a.N) == 64) {
    hipLaunchKernelGGL(prepare_kernel<64>, dim3(a.B), dim3(64), lay.bytes, st, k);
  } else {
    hipLaunchKernelGGL(prepare_kernel<256>, dim3(a.B), dim3(256), lay.bytes, st, k);
  }
  return hipGetLastError();
}

}  // namespace acnqp
