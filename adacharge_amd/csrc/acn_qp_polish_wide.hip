// Wide-site polish kernel (acn_qp_polish_wide.hpp): instantiation and launchers.
#include "acn_qp_launch.hpp"
#include "acn_qp_polish_wide.hpp"

namespace acnqp {

hipError_t launch_polish_wide_list(int32_t* status, int32_t* saved, int32_t* list, int32_t* count, int B, hipStream_t st) {
  hipLaunchKernelGGL(polish_wide_list_kernel, dim3(1), dim3(kPolThreads), 0, st, status, saved, list, count, B);
  return hipGetLastError();
}

hipError_t launch_polish_wide_restore(int32_t* status, const int32_t* saved, const int32_t* list, const int32_t* count, int B, hipStream_t st) {
  hipLaunchKernelGGL(polish_wide_restore_kernel, dim3((unsigned)std::max(1, std::min((B + kPolThreads - 1) / kPolThreads, 64))), dim3(kPolThreads), 0,
                     st, status, saved, list, count, B);
  return hipGetLastError();
}

hipError_t launch_polish_wide(const PolishArgs& pa, double* slab, int grid, hipStream_t st) {
  const int nrow = pa.M + (pa.has_peak ? 1 : 0);
  if (!polish_wide_holds(pa.N, pa.Tm, pa.K, pa.Mg, nrow) || slab == nullptr || pa.alongside) return hipErrorInvalidValue;
  const PolishWideLayout L(pa.N, pa.Tm, pa.K, pa.Mg, nrow);
  if (pa.max_rows != L.max_rows || pa.max_sess != L.max_sess || pa.blk_doubles != pa.Tm * L.blk_one) return hipErrorInvalidValue;
  if (L.lds_bytes() > kPolWideLdsBytes) return hipErrorInvalidValue;
  const size_t lds = (size_t)L.lds_bytes();
  hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&polish_wide_kernel), lds);
  if (e != hipSuccess) return e;
  PolishWideArgs aw;
  aw.p = pa;
  aw.slab = slab;
  hipLaunchKernelGGL(polish_wide_kernel, dim3(polish_wide_grid(std::min(grid, pa.B))), dim3(kPolThreads), lds, st, aw);
  return hipGetLastError();
}

}  // namespace acnqp
