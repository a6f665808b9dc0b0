// The projections of the z-update, written once for the kernels that run the safeguarded Newton water-filling (stream,
// long, general): onto B = box + energy rows, onto the site rows' sets C, and the demand-charge prox.
//
// Part 1, the RULES: scalars in, scalars out -- no lane operation, no memory access, no layout (as acn_qp_check.hpp).
// A kernel gathers its sums (registers and DPP rows, or one thread's loop) and asks these functions what they mean.
// Restated independently in oracle/admm_ref.py (project_window, _prox_rows); tests/test_project_rules.py compiles
// Part 1 for the host, builds a scalar water-filling from nothing else and holds it against that twin.
// Part 2, the ROW FUNCTIONS of the stream / long register layout (one row per 16-lane DPP row, its periods the 16 lanes
// times CT column registers): device only, and only what both kernels could take without a register more -- the tau
// search of the demand-charge row.  project_row and the site-row tile stay lambdas of each kernel that call the rules:
// the register allocator wants the first as a by-value function in the stream kernel and as a by-reference closure in
// the long kernel (DESIGN.md 2.1 has the tables).  Loads and stores of the site-row state stay in the kernels.
//
// The wave and tiled kernels run another water-filling (active-set start, rcp_small, guard 60) and do not include this
// file; their copies of the infeasible-bounds test point here, as do the stream kernel's copies of that test and of the
// site-row switch (either rule costs it a vector register on an instantiation).
#pragma once
#include <cmath>

#include "acn_qp_check.hpp"

namespace acnqp {

// ======== Part 1: rules ===================================================================================================
// ---- init: the bounds of a session's window cannot meet its energy row (sl = sum lb, su = sum ub over the window) --------
template <typename real>
__host__ __device__ inline bool bounds_miss_energy_row(real sl, real su, real cap, bool eq, real proj_tol) {
  const real slack = (real)64 * proj_tol * fmax((real)1, fabs(cap));
  return sl > cap + slack || (eq && su < cap - slack);
}

// ---- water-filling of one window: z = clip(zh - m), m the root of g(m) = sum clip(zh - m) = cap -------------------------
constexpr int kFillRoot = 0, kFillAtUb = 2, kFillAtLb = 3, kFillNone = 4;   // root-find, pinned at ub, pinned at lb, nothing
template <typename real>
__host__ __device__ inline real fill_tol(real cap, real proj_tol) { return proj_tol * fmax((real)1, fabs(cap)); }
// s0 = sum of the box-clipped point, sl / su = sum lb / ub over the window; `live`: the window has periods
template <typename real>
__host__ __device__ inline int fill_mode(bool live, bool eq, real s0, real sl, real su, real cap, real tol) {
  const bool act = live && (eq ? fabs(s0 - cap) > tol : s0 > cap + tol);
  return !act ? kFillNone : ((eq && cap >= su) ? kFillAtUb : (cap <= sl ? kFillAtLb : kFillRoot));
}
// the bracket [min (zh - ub), max (zh - lb)] of the root (an inequality row's multiplier is >= 0) and the start inside it
template <typename real>
__host__ __device__ inline real fill_start(bool eq, real mu0, real& lo, real hi) {
  if (!eq && lo < 0) lo = 0;
  return fmin(fmax(mu0, lo), hi);
}
template <typename real>
__host__ __device__ inline bool fill_done(real d, real tol) { return fabs(d) <= tol; }
// one step of the safeguarded Newton search at m: d = g(m) - cap, nf = periods strictly inside their box (-g'(m));
// `need`: the row is still searching (fill_done not yet true) -- a finished row keeps (lo, hi, m)
template <typename real>
__host__ __device__ inline void fill_step(real& m, real d, real nf, real& lo, real& hi, bool need) {
  lo = (need && d > 0) ? m : lo;
  hi = (need && !(d > 0)) ? m : hi;
  real mn = nf > 0 ? m + d / nf : (real)0.5 * (lo + hi);
  if (!(mn > lo && mn < hi)) mn = (real)0.5 * (lo + hi);
  m = need ? mn : m;
}

// ---- site rows: one row's z from its pre-projection point.  `peak`: the period's limit of a kRowPeak row (big: none),
// `quad` = rho / (rho + lf), `soc_scale` = min(1, lim / |(re, im)|) of the row's pair -- each kernel computes its own
// (lim / sqrt or lim * rsqrt_nr: different bits).  kRowMax passes through: the horizon-wide prox below follows.
template <typename real>
__host__ __device__ inline real site_row_z(int ty, real zh, real lim, real peak, real quad, real soc_scale) {
  real zn = zh;
  if (ty == kRowBox) zn = fmin(zn, lim);
  else if (ty == kRowPeak) zn = fmin(zn, peak);
  else if (ty == kRowQuad) zn = zn * quad;
  else if (ty == kRowSocRe || ty == kRowSocIm) zn = zn * soc_scale;
  return zn;
}

// ---- demand charge: z_t = min(zh_t, max(tau, floor)), tau the root of sum_t (zh_t - tau)+ = cw = dc / rho (Newton on a
// convex piecewise-linear function from tau = vmax - cw).  One step: S = sum (zh_t - tau)+, nn = periods above tau;
// `fin`: stop and keep tau (converged, stationary, or `guard` steps beyond `guard_max`).
template <typename real> struct DcStep { real tn; bool fin; };
template <typename real>
__host__ __device__ inline DcStep<real> dc_tau_step(real tau, real S, real nn, real cw, real vmax, real proj_tol, int guard, int guard_max) {
  const real f = S - cw;
  const real tn = nn > (real)0 ? tau + f / nn : vmax - cw;
  const bool fin = fabs(f) <= proj_tol * fmax((real)1, cw) * (real)16 || tn == tau || guard > guard_max;
  return {tn, fin};
}

#ifdef __HIPCC__
// ======== Part 2: row functions (device; acn_qp_common.hpp's row_sum / row_min / row_max are in scope) ====================
// tau of the demand-charge row whose periods are the 16 lanes of the lane group(s) with `mine` set times the CT column
// registers zv (period 16 c + t, live below Tm); the other lane groups run along on their own rows.
template <int CT>
__device__ __attribute__((always_inline)) inline double dc_row_tau(const double (&zv)[CT], double cw, int t, int Tm, bool mine) {
  typedef double real;
  using M = Mfma<real>;
  real vmax_l = -M::big;
#pragma unroll
  for (int c = 0; c < CT; ++c) vmax_l = (16 * c + t < Tm) ? fmax(vmax_l, zv[c]) : vmax_l;
  const real vmax = row_max<real>(vmax_l);
  real tau = vmax - cw;
  bool need = mine;
  int guard = 0;
  while (__any(need)) {
    ++guard;
    real sl = 0, nl = 0;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const real dd = zv[c] - tau;
      const bool on = (16 * c + t < Tm) && dd > 0.0;
      sl += on ? dd : 0.0;
      nl += on ? 1.0 : 0.0;
    }
    const real S = row_sum<real>(sl), nn = row_sum<real>(nl);
    const DcStep<real> s = dc_tau_step<real>(tau, S, nn, cw, vmax, M::proj_tol, guard, 200);
    tau = (need && !s.fin) ? s.tn : tau;
    need = need && !s.fin;
  }
  return tau;
}
#endif   // __HIPCC__

}  // namespace acnqp
