// Plant kernel (acn_qp_plant.hpp): instantiations and launcher.
#include "acn_qp_plant.hpp"

namespace acnqp {

hipError_t launch_plant(const PlantArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (plant_threads(a.N) == 64) {
    hipLaunchKernelGGL(plant_kernel<64>, dim3(a.B), dim3(64), 0, st, a);
  } else {
    hipLaunchKernelGGL(plant_kernel<256>, dim3(a.B), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace acnqp
