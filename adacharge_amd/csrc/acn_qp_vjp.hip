// Adjoint KKT kernel (acn_qp_vjp.hpp): instantiations, table sizes and launcher.
#include "acn_qp_launch.hpp"
#include "acn_qp_vjp.hpp"

namespace acnqp {

bool vjp_tables(int N, int Tm, int K, int Mg, int nrow, VjpTables* t) {
  t->max_rows = polish_max_rows(nrow, Tm);
  t->max_sess = polish_max_sess(N, K);
  t->blk_doubles = polish_blocks_that_fit(N, Tm, Mg, nrow, t->max_sess, kLdsPerCu);
  return t->blk_doubles >= 2 * nrow * (2 * nrow + 1) / 2;
}

hipError_t launch_vjp(const VjpArgs& a, hipStream_t st) {
  if (a.N > 64 || a.Tm > 32 || a.K > kMaxK) return hipErrorInvalidValue;
  const int nrow = a.M + (a.has_peak ? 1 : 0);
  const PolishLds L(a.N, a.Tm, a.Mg, nrow, a.max_rows, a.blk_doubles, a.max_sess);
  const size_t lds = (size_t)L.total * sizeof(double);
  const bool small = a.Tm <= 16;
  hipError_t e = small ? ensure_dynamic_lds(reinterpret_cast<const void*>(&vjp_kernel<4>), lds)
                       : ensure_dynamic_lds(reinterpret_cast<const void*>(&vjp_kernel<8>), lds);
  if (e != hipSuccess) return e;
  if (small) hipLaunchKernelGGL(vjp_kernel<4>, dim3(a.B), dim3(kPolThreads), lds, st, a);
  else hipLaunchKernelGGL(vjp_kernel<8>, dim3(a.B), dim3(kPolThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace acnqp
