// Dual report (acnqp_duals_device / acnqp_duals_host, include/acn_qp.h): for an answer (x, y) of any solver kernel, the
// multipliers of the energy rows (mu) and of the rate bounds (z) and four KKT residuals of the full primal-dual point.
// Independent of the solver loop: it reads the problem statement, x, y, status and the site in the CALLER's units
// (SiteDev::Gabi / limabi, as the polish does) and nothing a solver kernel left behind.
//
//   g = pd_eff x + q + G'y,  v = x - g,  mu_s: sum_{window s} clip(v - mu_s, lb, ub) = cap_s,  z = -(g + mu_s)
//
// Two instantiations, chosen by the shape only (duals_wave_shape):
//   WAVE   N <= 64, horizon <= 16: one wavefront per problem (a workgroup of one wave: its barriers never wait for another
//          wave), lane = EVSE in the session phase (the layout of the wave kernel).  x, g, lb, ub are staged in LDS with
//          coalesced loads -- a lane walking its own row in global memory touches one cache line per lane and
//          instruction, which made the texture path the bottleneck (16,384 x 54 x 12: 1.19 ms, against 0.57 ms now)
//   block  everything else: one workgroup per problem, g formed by all threads in the z output (or a scratch of the
//          same shape when z is not wanted), then one thread per EVSE
// Work per problem: one G' product, one exact water-filling per session, one G product for the site rows -- about one
// ADMM iteration.
//
// Determinism: every sum runs in a fixed order inside ONE thread (G'y over the rows, a window over its periods, a site
// row over the EVSEs); threads are combined by max only.  No atomics.  The same problem gives the same bits in any
// batch and at any position.  tests/duals_spec.py restates it in numpy, sum for sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "acn_qp_common.hpp"

namespace acnqp {

struct DualsArgs {
  int B, N, Tm, K, M, Mg, cone, has_peak, has_flat, has_max;
  const double* G;        // [Mg][N] acnqp_site.G as given
  const double* limits;   // [M]
  const int32_t* horizon;
  const double *lb, *ub, *q, *pdiag;
  const int32_t *s_off, *s_len;
  const double* s_cap;
  const uint8_t* s_eq;
  const double *peak, *lf, *dc;
  const double *x, *y;
  const int32_t* status;  // or nullptr: all solved
  double *mu, *z, *res;   // z may be nullptr
  double* gbuf;           // [B][N][Tm]: == z when z is wanted, else scratch
  double reg_rel;
};

constexpr double kDualsInf = __builtin_huge_val();

__device__ inline double duals_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// max over the group: the wavefront (WAVE) or the workgroup (`red`: one double per wave; two barriers)
template <bool WAVE>
__device__ inline double duals_group_max(double v, double* red) {
  v = duals_wave_max(v);
  if (WAVE) return v;
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double m = red[0];
  for (int k = 1; k < nw; ++k) m = fmax(m, red[k]);
  __syncthreads();
  return m;
}

// The shift mu with sum_t clip(v_t - mu, lb_t, ub_t) = cap over one window of L periods (v = x - g), exactly: a
// safeguarded Newton iteration over the SEGMENTS of the piecewise-linear sum -- every step looks at the segment that
// holds the trial point, solves that segment's linear equation, and either ends there (the root lies on it) or drops
// the segment from the bracket -- so it ends after at most 2 L + 1 steps on the segment that holds the root.
// Ties (no free entry, the sum of bounds equal to cap): the admissible value of least magnitude.  A cap beyond the bounds
// counts as reached at the nearest end.  tests/duals_spec.py::waterfill, statement for statement.
__device__ inline double duals_waterfill(const double* __restrict__ x, const double* __restrict__ g,
                                         const double* __restrict__ lb, const double* __restrict__ ub, int L, double cap, bool eq) {
  double f0 = 0, f_hi = 0, f_lo = 0, bmin = kDualsInf, bmax = -kDualsInf;
  for (int t = 0; t < L; ++t) {
    const double l = lb[t], u = fmax(ub[t], l), v = x[t] - g[t];
    f0 += fmin(fmax(v, l), u);
    f_hi += u;
    f_lo += l;
    if (u > l) {
      bmin = fmin(bmin, v - u);
      bmax = fmax(bmax, v - l);
    }
  }
  if (!eq && f0 <= cap) return 0.0;
  if (cap >= f_hi) return fmin(0.0, bmin);
  if (cap <= f_lo) return fmax(0.0, bmax);
  double lo = bmin, hi = bmax;   // sum(lo) = f_hi > cap > f_lo = sum(hi)
  double m = (lo < 0.0 && 0.0 < hi) ? 0.0 : 0.5 * (lo + hi);
  for (int it = 0; it < 2 * L + 8; ++it) {
    double sv = 0, sb = 0, below = lo, above = hi;
    int nf = 0;
    for (int t = 0; t < L; ++t) {
      const double l = lb[t], u = fmax(ub[t], l), v = x[t] - g[t];
      const double bu = v - u, bl = v - l;
      if (u > l) {
        if (bu <= m) below = fmax(below, bu); else above = fmin(above, bu);
        if (bl <= m) below = fmax(below, bl); else above = fmin(above, bl);
      }
      if (m < bu) sb += u;
      else if (m >= bl) sb += l;
      else { sv += v; ++nf; }
    }
    bool up;
    double r = 0;
    if (nf > 0) {
      r = ((sv + sb) - cap) / (double)nf;
      if (below <= r && r <= above) return r;
      up = r > above;
    } else {
      const double d = sb - cap;
      if (d == 0.0) return fmin(fmax(0.0, below), above);
      up = d > 0.0;
    }
    if (up) lo = above; else hi = below;
    m = (nf > 0 && lo < r && r < hi) ? r : 0.5 * (lo + hi);
    if (!(lo < m && m < hi)) return lo;
  }
  return m;
}

template <bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 1024) void duals_kernel(const DualsArgs A) {
  __shared__ double red[16];
  extern __shared__ double duals_lds[];   // WAVE: x, g, lb, ub of the problem, rows padded to an odd length
  const int gs = WAVE ? 64 : (int)blockDim.x;
  const int gt = (int)threadIdx.x;
  const int b = (int)blockIdx.x;
  const int N = A.N, Tm = A.Tm, K = A.K, M = A.M, Mg = A.Mg;
  const size_t n = (size_t)N * Tm;
  const double* lb = A.lb + (size_t)b * n;
  const double* ub = A.ub + (size_t)b * n;
  const double* q = A.q + (size_t)b * n;
  const double* x = A.x + (size_t)b * n;
  const double* y = A.y + (size_t)b * Mg * Tm;   // (never dereferenced when Mg == 0)
  double* zo = A.z ? A.z + (size_t)b * n : nullptr;
  double* muo = A.mu + (size_t)b * K * N;

  const int st = A.status ? A.status[b] : 1;
  if (st != 1 && st != 5) {   // not an answer: zeros and +inf (the whole workgroup leaves)
    for (int k = gt; k < K * N; k += gs) muo[k] = 0.0;
    if (zo) for (size_t k = gt; k < n; k += gs) zo[k] = 0.0;
    if (gt < 4) A.res[(size_t)b * 4 + gt] = kDualsInf;
    return;
  }

  // where the session phase reads x, g, lb, ub (row stride ld) and writes z: LDS (WAVE) or global memory
  const int ld = WAVE ? (Tm | 1) : Tm;
  double* sx = duals_lds;
  double* sg = sx + (size_t)N * ld;
  double* sl = sg + (size_t)N * ld;
  double* su = sl + (size_t)N * ld;
  const double* rx = WAVE ? sx : x;
  const double* rl = WAVE ? sl : lb;
  const double* ru = WAVE ? su : ub;
  double* rg = WAVE ? sg : A.gbuf + (size_t)b * n;
  double* rz = WAVE ? sg : zo;   // (z overwrites g entry by entry; WAVE copies it out at the end)

  // ---- |q|_inf, max(ub), the effective diagonal ------------------------------------------------------------------
  double qm = 0, um = -kDualsInf;
  for (size_t k = gt; k < n; k += gs) {
    const double lv = lb[k], uv = ub[k];
    qm = fmax(qm, fabs(q[k]));
    um = fmax(um, fmax(uv, lv));
    if (WAVE) {
      const int i = (int)(k / Tm), t = (int)(k - (size_t)i * Tm);
      sx[i * ld + t] = x[k];
      sg[i * ld + t] = q[k];   // (q until g replaces it)
      sl[i * ld + t] = lv;
      su[i * ld + t] = uv;
    }
  }
  const double qn = duals_group_max<WAVE>(qm, red);
  const double ubmax = duals_group_max<WAVE>(um, red);
  const bool has_prox = (A.has_flat && A.lf[b] > 0.0) || (A.has_max && A.dc[b] > 0.0);
  const double pd = effective_pdiag<double>(A.pdiag[b], A.reg_rel, qn, ubmax, A.horizon[b], has_prox);
  const double qs = fmax(1.0, qn);
  const int T = A.horizon[b];

  // ---- g = pd x + q + G'y (rows of G in order) ---------------------------------------------------------------------
  for (size_t k = gt; k < n; k += gs) {
    const int i = (int)(k / Tm), t = (int)(k - (size_t)i * Tm);
    double acc = 0;
#pragma unroll 8
    for (int j = 0; j < Mg; ++j) acc += A.G[(size_t)j * N + i] * y[(size_t)j * Tm + t];
    const double xk = WAVE ? sx[i * ld + t] : x[k], qk = WAVE ? sg[i * ld + t] : q[k];
    rg[(size_t)i * ld + t] = pd * xk + qk + acc;
  }
  // (WAVE: the workgroup is ONE wavefront -- this orders its LDS writes before the reads of other lanes and never waits
  //  for another wave; block form: workgroup-scope release / acquire of g in global memory)
  __syncthreads();

  // ---- one thread per EVSE: its sessions in period order, the entries outside every window -------------------------
  const bool eq = A.s_eq[b] != 0;
  double stat = 0, energy = 0;
  for (int i = gt; i < N; i += gs) {
    const size_t row = (size_t)i * ld;
    for (int k = 0; k < K; ++k) muo[(size_t)k * N + i] = 0.0;
    int t = 0;
    while (t < Tm) {
      int ks = -1, w0 = 0, w1 = 0;
      for (int k = 0; k < K; ++k) {   // the window that holds t (windows of one EVSE are disjoint)
        const size_t sidx = ((size_t)b * K + k) * N + i;
        const int len = A.s_len[sidx];
        if (len <= 0) continue;
        const int off = A.s_off[sidx];
        const int a0 = off > 0 ? off : 0;
        const int a1 = (long long)off + len < (long long)Tm ? off + len : Tm;
        if (t >= a0 && t < a1) { ks = k; w0 = a0; w1 = a1; break; }
      }
      if (ks < 0) {   // outside every window: the box alone
        const double l = rl[row + t], u = fmax(ru[row + t], l), xv = rx[row + t];
        const double v = xv - rg[row + t];
        stat = fmax(stat, fabs(xv - fmin(fmax(v, l), u)));
        if (rz) rz[row + t] = 0.0;
        ++t;
        continue;
      }
      const double cap = A.s_cap[((size_t)b * K + ks) * N + i];
      const double m = duals_waterfill(rx + row + w0, rg + row + w0, rl + row + w0, ru + row + w0, w1 - w0, cap, eq);
      muo[(size_t)ks * N + i] = m;
      double e = 0;
      for (int tt = w0; tt < w1; ++tt) {
        const double l = rl[row + tt], u = fmax(ru[row + tt], l), xv = rx[row + tt], gv = rg[row + tt];
        const double v = xv - gv;
        stat = fmax(stat, fabs(xv - fmin(fmax(v - m, l), u)));
        e += xv;
        if (rz) rz[row + tt] = tt < T ? -(gv + m) : 0.0;
      }
      const double viol = eq ? fabs(e - cap) : fmax(e - cap, 0.0);
      energy = fmax(energy, viol / fmax(1.0, fabs(cap)));
      t = w1;
    }
  }
  if (WAVE && zo) {   // z out of LDS, coalesced
    __syncthreads();
    for (size_t k = gt; k < n; k += gs) {
      const int i = (int)(k / Tm), t = (int)(k - (size_t)i * Tm);
      zo[k] = sg[i * ld + t];
    }
  }

  // ---- site rows: violation and multiplier x slack (sums over the EVSEs in order) -----------------------------------
  double site = 0, comp = 0;
  const bool soc = A.cone == 1;
  for (int k = gt; k < M * Tm; k += gs) {
    const int c = k / Tm, t = k - c * Tm;
    double a = 0, a2 = 0;
#pragma unroll 8
    for (int i = 0; i < N; ++i) a += A.G[(size_t)c * N + i] * rx[(size_t)i * ld + t];
    double lam = y[(size_t)c * Tm + t];
    if (soc) {
#pragma unroll 8
      for (int i = 0; i < N; ++i) a2 += A.G[(size_t)(c + M) * N + i] * rx[(size_t)i * ld + t];
      a = hypot(a, a2);
      lam = hypot(lam, y[(size_t)(c + M) * Tm + t]);
    }
    const double lim = A.limits[c], sl = lim - a, sc = fmax(1.0, lim);
    site = fmax(site, fmax(-sl, 0.0) / sc);
    comp = fmax(comp, lam * fabs(sl) / sc / qs);
  }
  if (A.has_max) {   // demand-charge row: y_t (max_t v'x_t - v'x_t)
    const int r = Mg - 1 - (A.has_peak ? 1 : 0);
    double top = -kDualsInf;
    for (int t = gt; t < Tm; t += gs) {
      double a = 0;
      for (int i = 0; i < N; ++i) a += A.G[(size_t)r * N + i] * rx[(size_t)i * ld + t];
      top = fmax(top, a);
    }
    top = duals_group_max<WAVE>(top, red);
    for (int t = gt; t < Tm; t += gs) {
      double a = 0;
      for (int i = 0; i < N; ++i) a += A.G[(size_t)r * N + i] * rx[(size_t)i * ld + t];
      comp = fmax(comp, y[(size_t)r * Tm + t] * (top - a) / (qs * fmax(1.0, fabs(top))));
    }
  }
  if (A.has_peak) {
    const int r = Mg - 1;
    for (int t = gt; t < Tm; t += gs) {
      const double pk = A.peak[(size_t)b * Tm + t];
      if (!(fabs(pk) < kDualsInf)) continue;   // unlimited period
      double a = 0;
      for (int i = 0; i < N; ++i) a += A.G[(size_t)r * N + i] * rx[(size_t)i * ld + t];
      const double sl = pk - a, sc = fmax(1.0, fabs(pk));
      site = fmax(site, fmax(-sl, 0.0) / sc);
      comp = fmax(comp, y[(size_t)r * Tm + t] * fabs(sl) / sc / qs);
    }
  }
  stat = duals_group_max<WAVE>(stat, red);
  energy = duals_group_max<WAVE>(energy, red);
  site = duals_group_max<WAVE>(site, red);
  comp = duals_group_max<WAVE>(comp, red);
  if (gt == 0) {
    double* r = A.res + (size_t)b * 4;
    r[0] = stat; r[1] = energy; r[2] = site; r[3] = comp;
  }
}

// which instantiation serves a shape: a function of the shape only (WAVE: x, g, lb, ub in LDS, at most 35 KB)
constexpr int kDualsWaveTm = 16;
inline bool duals_wave_shape(int N, int Tm) { return N <= 64 && Tm <= kDualsWaveTm; }
inline size_t duals_wave_lds(int N, int Tm) { return (size_t)4 * N * (Tm | 1) * sizeof(double); }
hipError_t launch_duals(const DualsArgs& a, hipStream_t st);

}  // namespace acnqp
