// Site data of a handle: the site's rows in the kernels' internal order, equilibrated, eigen-decomposed and uploaded
// (acnqp_create).  Host code of the API translation unit (acn_qp_api.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "acn_qp.h"
#include "acn_qp_common.hpp"
#include "acn_qp_rank.hpp"
#include "acn_qp_route.hpp"

namespace acnqp {

// Cyclic Jacobi eigen-decomposition of a small symmetric matrix (n <= 48).
// a is overwritten; on return lam[k] are eigenvalues and V[r*n + k] the k-th eigenvector.
inline void jacobi_eigh(int n, std::vector<double>& a, std::vector<double>& lam, std::vector<double>& V) {
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0, diag = 0;
    for (int p = 0; p < n; ++p)
      for (int q = 0; q < n; ++q) (p == q ? diag : off) += a[(size_t)p * n + q] * a[(size_t)p * n + q];
    if (off <= 1e-32 * (diag > 0 ? diag : 1.0)) break;
    for (int p = 0; p < n - 1; ++p) {
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq;
          a[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk;
          a[(size_t)q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = c * vkp - s * vkq;
          V[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
    }
  }
  lam.resize(n);
  for (int i = 0; i < n; ++i) lam[i] = a[(size_t)i * n + i];
}

// Site data in the kernels' internal row order (SOC pairs sit in adjacent registers of one lane).
struct SiteDev {
  bool ready = false;
  int MR = 0;                    // padded rows (multiple of 16)
  double peak_scale = 1, flat_scale = 1, max_scale = 1;   // row-equilibration factors of the prox rows
  void *G = nullptr, *Ghat = nullptr, *Q = nullptr, *lam = nullptr, *rowlim = nullptr;
  void *fragG = nullptr, *fragQ = nullptr;   // Ghat / Q in MFMA A-operand fragment order (tiled kernel)
  void *fragG2 = nullptr, *fragQ2 = nullptr; // the same with the four k-slices of a fragment as two adjacent pairs per lane (long-horizon kernel)
  // the wave kernel's own copies in the compacted eigenbasis (acn_qp_rank.hpp: live eigenpairs first); no other kernel reads them
  void *GhatW = nullptr, *lamW = nullptr, *fragQW = nullptr;
  int rank = 0, eig_ksteps = 0;  // live eigenpairs, and the MFMA k-steps that hold them once compacted
  int32_t* rowtype = nullptr;
  int32_t* rowabi = nullptr;     // internal row -> row of acnqp_site.G (-1: padding)
  void* rowscale = nullptr;      // equilibration factor of each internal row
  double *Gabi = nullptr, *limabi = nullptr;   // acnqp_site.G / limits as the caller gave them (the polish kernel works in the caller's units)
  void release() {
    if (Gabi) (void)hipFree(Gabi);
    if (limabi) (void)hipFree(limabi);
    Gabi = limabi = nullptr;
    for (void** p : {&G, &Ghat, &Q, &lam, &rowlim, &fragG, &fragQ, &fragG2, &fragQ2, &rowscale, &GhatW, &lamW, &fragQW}) { if (*p) (void)hipFree(*p); *p = nullptr; }
    if (rowtype) (void)hipFree(rowtype);
    if (rowabi) (void)hipFree(rowabi);
    rowtype = nullptr; rowabi = nullptr;
    ready = false;
  }
};

// internal row slot of site row (constraint c, component) -- see acn_qp_tiled.hpp
inline int soc_slot(int c, int im) { return 8 * (c / 4) + (c % 4) + 4 * im; }

// `h`: the site's shape (MR from padded_rows, acn_qp_route.hpp); G, limits: acnqp_site's, in ABI order.  Returns
// ACNQP_OK or an ACNQP_ERR_* with its text in *err.
inline int build_site_dev(const SiteShape* h, const std::vector<double>& G, const std::vector<double>& limits, SiteDev* d,
                          std::string* err) {
  const int N = h->N, M = h->M, NP = h->NP(), MR = h->MR;
  if (MR > 48) { *err = "site has too many rows for the tiled kernel (> 48 after padding)"; return ACNQP_ERR_INVALID; }
  std::vector<double> Gi((size_t)MR * NP, 0.0), lim(MR, 0.0);
  std::vector<int32_t> ty(MR, acnqp::kRowFree), abi(MR, -1);
  auto put = [&](int slot, int src_row, int type, double limit) {
    for (int i = 0; i < N; ++i) Gi[(size_t)slot * NP + i] = G[(size_t)src_row * N + i];
    abi[slot] = src_row;
    ty[slot] = type;
    lim[slot] = limit;
  };
  int peak_slot;   // first slot after the infrastructure rows: flat row (if any), then peak row
  if (h->cone == ACNQP_CONE_SOC) {
    for (int c = 0; c < M; ++c) {
      put(soc_slot(c, 0), c, acnqp::kRowSocRe, limits[c]);
      put(soc_slot(c, 1), c + M, acnqp::kRowSocIm, limits[c]);
    }
    peak_slot = 8 * ((M + 3) / 4);
  } else {
    for (int c = 0; c < M; ++c) put(c, c, acnqp::kRowBox, limits[c]);
    peak_slot = M;
  }
  int flat_slot = -1, max_slot = -1, pk_slot = -1;
  if (h->has_flat) { flat_slot = peak_slot; put(peak_slot, h->Mg - 1 - h->has_peak - h->has_max, acnqp::kRowQuad, 0.0); ++peak_slot; }
  if (h->has_max) { max_slot = peak_slot; put(peak_slot, h->Mg - 1 - h->has_peak, acnqp::kRowMax, 0.0); ++peak_slot; }
  if (h->has_peak) { pk_slot = peak_slot; put(peak_slot, h->Mg - 1, acnqp::kRowPeak, 0.0); }

  // Row equilibration (solver-internal, invisible at the ABI): every site row -- a SOC pair counts as
  // one row -- is scaled by 1/sqrt(|g|_2), and its limit with it.  The constraint set is unchanged;
  // the ADMM penalty now weighs a 26-EVSE feeder row and a 8-EVSE pod row alike, which roughly
  // halves the iteration count (measured on the Caltech-shaped network).
  std::vector<double> rs(MR, 1.0);
  for (int j = 0; j < MR; ++j) {
    if (ty[j] == acnqp::kRowFree || ty[j] == acnqp::kRowSocIm) continue;
    double n2 = 0;
    const int j2 = ty[j] == acnqp::kRowSocRe ? j + 4 : -1;
    for (int i = 0; i < N; ++i) {
      n2 += Gi[(size_t)j * NP + i] * Gi[(size_t)j * NP + i];
      if (j2 >= 0) n2 += Gi[(size_t)j2 * NP + i] * Gi[(size_t)j2 * NP + i];
    }
    const double sc = n2 > 0 ? 1.0 / std::sqrt(std::sqrt(n2)) : 1.0;
    rs[j] = sc;
    if (j2 >= 0) rs[j2] = sc;
  }
  for (int j = 0; j < MR; ++j) {
    for (int i = 0; i < N; ++i) Gi[(size_t)j * NP + i] *= rs[j];
    lim[j] *= rs[j];
  }
  d->flat_scale = flat_slot >= 0 ? rs[flat_slot] : 1.0;
  d->max_scale = max_slot >= 0 ? rs[max_slot] : 1.0;
  d->peak_scale = pk_slot >= 0 ? rs[pk_slot] : 1.0;

  std::vector<double> GGt((size_t)MR * MR, 0.0), lam, Q;
  for (int r = 0; r < MR; ++r)
    for (int c = 0; c < MR; ++c) {
      double s = 0;
      for (int i = 0; i < N; ++i) s += Gi[(size_t)r * NP + i] * Gi[(size_t)c * NP + i];
      GGt[(size_t)r * MR + c] = s;
    }
  jacobi_eigh(MR, GGt, lam, Q);
  double lmax = 0;
  for (int k = 0; k < MR; ++k) lmax = std::fmax(lmax, lam[k]);
  std::vector<double> Gh((size_t)MR * NP, 0.0);
  for (int k = 0; k < MR; ++k) {
    if (lam[k] < 1e-12 * std::fmax(1.0, lmax)) { lam[k] = 0.0; continue; }
    for (int i = 0; i < N; ++i) {
      double s = 0;
      for (int r = 0; r < MR; ++r) s += Q[(size_t)r * MR + k] * Gi[(size_t)r * NP + i];
      Gh[(size_t)k * NP + i] = s;
    }
  }
  auto up = [&](void** dst, const std::vector<double>& src) -> hipError_t {
    hipError_t e = hipMalloc(dst, src.size() * sizeof(double));
    if (e != hipSuccess) return e;
    return hipMemcpy(*dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice);
  };
  // MFMA A-operand fragments in the order the tiled and the large-site kernel read them (one coalesced
  // 64-lane row per fragment register): see acn_qp_tiled.hpp / acn_qp_stream.hpp.  NP / 16 EVSE tiles.
  std::vector<double> fragG, fragQ;
  const int NWv = NP / 16, MT = MR / 16;
  auto frag_of_Q = [&](const std::vector<double>& Qm) {   // [mo][mi][0]: Q' (eigen tile mo x row tile mi), [..][1]: Q (row tile mo x eigen tile mi)
    std::vector<double> f((size_t)MT * MT * 2 * 4 * 64, 0.0);
    for (int lane = 0; lane < 64; ++lane) {
      const int g = lane >> 4, t = lane & 15;
      for (int sI = 0; sI < 4; ++sI) {
        const int ro = acnqp::Mfma<double>::rowof(g, sI);
        for (int m = 0; m < MT; ++m)
          for (int mi = 0; mi < MT; ++mi) {   // m plays the role of mo
            f[((((size_t)m * MT + mi) * 2 + 0) * 4 + sI) * 64 + lane] = Qm[(size_t)(16 * mi + ro) * MR + 16 * m + t];
            f[((((size_t)m * MT + mi) * 2 + 1) * 4 + sI) * 64 + lane] = Qm[(size_t)(16 * m + t) * MR + 16 * mi + ro];
          }
      }
    }
    return f;
  };
  {
    fragG.assign((size_t)NWv * MT * 2 * 4 * 64, 0.0);
    for (int lane = 0; lane < 64; ++lane) {
      const int g = lane >> 4, t = lane & 15;
      for (int sI = 0; sI < 4; ++sI) {
        const int ro = acnqp::Mfma<double>::rowof(g, sI);
        for (int m = 0; m < MT; ++m)
          for (int w = 0; w < NWv; ++w) {
            fragG[((((size_t)w * MT + m) * 2 + 0) * 4 + sI) * 64 + lane] = Gh[(size_t)(16 * m + t) * NP + 16 * w + ro];
            fragG[((((size_t)w * MT + m) * 2 + 1) * 4 + sI) * 64 + lane] = Gh[(size_t)(16 * m + ro) * NP + 16 * w + t];
          }
      }
    }
    fragQ = frag_of_Q(Q);
  }
  // the wave kernel's copies: eigenpair perm[k] in slot k (Ghat's rows, lam, Q's columns)
  const EigRank er = eig_rank(lam);
  std::vector<double> GhW((size_t)MR * NP), lamW(MR), QW((size_t)MR * MR);
  for (int k = 0; k < MR; ++k) {
    const int src = er.perm[k];
    lamW[k] = lam[src];
    for (int i = 0; i < NP; ++i) GhW[(size_t)k * NP + i] = Gh[(size_t)src * NP + i];
    for (int r = 0; r < MR; ++r) QW[(size_t)r * MR + k] = Q[(size_t)r * MR + src];
  }
  d->rank = er.rank;
  d->eig_ksteps = er.eig_ksteps;
  hipError_t e = up(&d->G, Gi);
  if (e == hipSuccess && !fragG.empty()) e = up(&d->fragG, fragG);
  if (e == hipSuccess && !fragQ.empty()) e = up(&d->fragQ, fragQ);
  {
    // pair order: [k-slice / 2][lane][k-slice % 2] inside every 4 x 64 fragment block (one 16-byte load per lane
    // fetches two k-slices: acn_qp_long.hpp)
    auto paired = [](const std::vector<double>& in) {
      std::vector<double> out(in.size());
      for (size_t blk = 0; blk + 256 <= in.size(); blk += 256)
        for (int sI = 0; sI < 4; ++sI)
          for (int lane = 0; lane < 64; ++lane) out[blk + (size_t)(sI >> 1) * 128 + lane * 2 + (sI & 1)] = in[blk + (size_t)sI * 64 + lane];
      return out;
    };
    if (e == hipSuccess && !fragG.empty()) e = up(&d->fragG2, paired(fragG));
    if (e == hipSuccess && !fragQ.empty()) e = up(&d->fragQ2, paired(fragQ));
  }
  if (e == hipSuccess) e = up(&d->Ghat, Gh);
  if (e == hipSuccess) e = up(&d->Q, Q);
  if (e == hipSuccess) e = up(&d->lam, lam);
  if (e == hipSuccess) e = up(&d->GhatW, GhW);
  if (e == hipSuccess) e = up(&d->lamW, lamW);
  if (e == hipSuccess) e = up(&d->fragQW, frag_of_Q(QW));
  if (e == hipSuccess) e = up(&d->rowlim, lim);
  if (e == hipSuccess) e = up(&d->rowscale, rs);
  if (e == hipSuccess) e = hipMalloc((void**)&d->rowtype, MR * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(d->rowtype, ty.data(), MR * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&d->rowabi, MR * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(d->rowabi, abi.data(), MR * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&d->Gabi, std::max<size_t>(G.size(), 1) * sizeof(double));
  if (e == hipSuccess && !G.empty()) e = hipMemcpy(d->Gabi, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc((void**)&d->limabi, std::max<size_t>(limits.size(), 1) * sizeof(double));
  if (e == hipSuccess && !limits.empty()) e = hipMemcpy(d->limabi, limits.data(), limits.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { d->release(); *err = std::string("site upload: ") + hipGetErrorString(e); return ACNQP_ERR_HIP; }
  d->MR = MR;
  d->ready = true;
  return ACNQP_OK;
}

}  // namespace acnqp
