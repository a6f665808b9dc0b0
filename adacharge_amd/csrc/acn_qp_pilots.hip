// Pilot-signal kernel (acn_qp_pilots.hpp): instantiations and launcher.
#include "acn_qp_pilots.hpp"

namespace acnqp {

hipError_t launch_pilots(const PilotsArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  PilotsArgs k = a;
  const PilotsLayout lay = pilots_layout(a.N, a.M, a.L, a.mode);
  k.site_lds = lay.site_lds;
  k.levels_lds = lay.levels_lds;
  if (pilots_threads(a.N) == 64) {
    hipLaunchKernelGGL(pilots_kernel<64>, dim3(a.B), dim3(64), lay.bytes, st, k);
  } else {
    hipLaunchKernelGGL(pilots_kernel<256>, dim3(a.B), dim3(256), lay.bytes, st, k);
  }
  return hipGetLastError();
}

}  // namespace acnqp
