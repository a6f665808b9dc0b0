// Rank analysis of a site's eigen-decomposition, for the wave-per-problem kernel (acn_qp_wave.hpp).  build_site_dev
// (acn_qp_site.hpp) sets every eigenvalue of G G' below 1e-12 lam_max to exactly 0 and leaves that row of Ghat all
// zeros.  Such a NULL eigen-row k stays out of every iteration's result: g0[k] = (Ghat r0)[k] = 0, h^[k] = (g0[k] +
// lam_k e^[k]) / a = 0, and e^[k] = w^[k] is only ever multiplied by the zero row Ghat[k, :].  The wave kernel therefore
// works in a COMPACTED eigenbasis -- live eigenpairs first, in the order the Jacobi sweeps left them -- and runs its
// eigen-side MFMA chains over the live k-steps only (four eigen-rows per v_mfma_f64_16x16x4 k-step).  The live terms of
// every sum keep their order, a skipped term was finite x 0: the results are the same bits.
// Host code only: no HIP, no handle, no getenv -- tests/test_wave_rank.py compiles this header with the host compiler.
#pragma once
#include <vector>

namespace acnqp {

struct EigRank {
  std::vector<int> perm;   // slot k' of the compacted basis holds eigenpair perm[k']: a stable partition, live first
  int rank = 0;            // live eigenpairs (lam > 0 after the zeroing)
  int eig_ksteps = 0;      // MFMA k-steps that hold a live eigen-row once compacted: ceil(rank / 4)
};

// lam: the eigenvalues AFTER build_site_dev's zeroing (a null one is exactly 0)
inline EigRank eig_rank(const std::vector<double>& lam) {
  EigRank e;
  const int n = (int)lam.size();
  e.perm.reserve(n);
  for (int k = 0; k < n; ++k)
    if (lam[k] != 0.0) e.perm.push_back(k);
  e.rank = (int)e.perm.size();
  for (int k = 0; k < n; ++k)
    if (lam[k] == 0.0) e.perm.push_back(k);
  e.eig_ksteps = (e.rank + 3) / 4;
  return e;
}

// The eigen extents (live k-steps) the wave kernel is instantiated with besides the full one: what the sites of
// BASELINE.json need (ranks 5 ... 11).  One eigen tile at most: a rank above 16 takes the full extent.
constexpr int kWaveExtentSmall = 2, kWaveExtentMid = 3;

// The extent of the instantiation that serves a site: the smallest specialised one that holds its live k-steps, or 0 --
// the full extent of MR / 4 k-steps on the original eigenbasis, i.e. the kernel as it was.  A function of the site only.
// full_rank: the diagnostic switch ACNQP_WAVE_FULL_RANK=1.
inline int wave_eig_extent(int eig_ksteps, bool full_rank) {
  if (full_rank) return 0;
  if (eig_ksteps <= kWaveExtentSmall) return kWaveExtentSmall;
  if (eig_ksteps <= kWaveExtentMid) return kWaveExtentMid;
  return 0;
}

// The EVSE extent of P = Ghat r0: the chain sums over the EVSEs, four per MFMA k-step, and a site of N <= 64 EVSEs fills
// ceil(N / 4) of the 16 k-steps; beyond them the scratch rows and the columns of Ghat are zeros for good.  The wave kernel
// is instantiated for 14 k-steps (N <= 56: caltech54, jpl52) and for all 16.  A function of the site's N only, never of
// the batch.  full_evse: the diagnostic switch ACNQP_WAVE_FULL_EVSE=1.
constexpr int kWaveEvseKsteps = 16, kWaveEvseExtent = 14;

inline int wave_evse_extent(int N, bool full_evse) {
  const int ks = (N + 3) / 4;
  return !full_evse && ks <= kWaveEvseExtent ? kWaveEvseExtent : kWaveEvseKsteps;
}

}  // namespace acnqp
