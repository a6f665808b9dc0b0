// Long-horizon adjoint KKT kernel (acn_qp_vjp_long.hpp): instantiation, grid and launcher.
#include "acn_qp_launch.hpp"
#include "acn_qp_vjp_long.hpp"

namespace acnqp {

int vjp_long_grid(int N, int Tm, int K, int Mg, int nrow, int batch, int cus) {
  const long long fit = kVjpLongScratchBytes / PolishLongLayout(N, Tm, K, Mg, nrow).slab_bytes();
  return (int)std::max(1ll, std::min<long long>(std::min(batch, std::max(cus, 1)), fit));
}

hipError_t launch_vjp_long(const VjpArgs& a, double* slab, int grid, hipStream_t st) {
  const int nrow = a.M + (a.has_peak ? 1 : 0);
  if (!polish_long_holds(a.N, a.Tm, a.K, a.Mg, nrow) || a.K > kMaxK || slab == nullptr || grid < 1) return hipErrorInvalidValue;
  const PolishLongLayout L(a.N, a.Tm, a.K, a.Mg, nrow);
  if (a.max_rows != L.max_rows || a.max_sess != L.max_sess || a.blk_doubles != a.Tm * L.blk_one) return hipErrorInvalidValue;
  const size_t lds = (size_t)L.lds_bytes();
  hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&vjp_long_kernel), lds);
  if (e != hipSuccess) return e;
  VjpLongArgs al;
  al.v = a;
  al.slab = slab;
  hipLaunchKernelGGL(vjp_long_kernel, dim3(std::min(grid, a.B)), dim3(kPolThreads), lds, st, al);
  return hipGetLastError();
}

}  // namespace acnqp
