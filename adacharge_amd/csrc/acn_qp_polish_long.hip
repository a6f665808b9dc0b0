// Long-horizon polish kernel (acn_qp_polish_long.hpp): instantiation and launcher.
#include "acn_qp_launch.hpp"
#include "acn_qp_polish_long.hpp"

namespace acnqp {

hipError_t launch_polish_long(const PolishArgs& pa, double* slab, int grid, hipStream_t st) {
  const int nrow = pa.M + (pa.has_peak ? 1 : 0);
  if (!polish_long_holds(pa.N, pa.Tm, pa.K, pa.Mg, nrow) || slab == nullptr || pa.alongside) return hipErrorInvalidValue;
  const PolishLongLayout L(pa.N, pa.Tm, pa.K, pa.Mg, nrow);
  if (pa.max_rows != L.max_rows || pa.max_sess != L.max_sess || pa.blk_doubles != pa.Tm * L.blk_one) return hipErrorInvalidValue;
  const size_t lds = (size_t)L.lds_bytes();
  hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&polish_long_kernel), lds);
  if (e != hipSuccess) return e;
  PolishLongArgs al;
  al.p = pa;
  al.slab = slab;
  hipLaunchKernelGGL(polish_long_kernel, dim3(polish_long_grid(std::min(grid, pa.B))), dim3(kPolThreads), lds, st, al);
  return hipGetLastError();
}

}  // namespace acnqp
