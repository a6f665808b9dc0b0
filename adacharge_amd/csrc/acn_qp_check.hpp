// The rules of the residual check, written once for all five solver kernels (wave, tiled, stream, long, general):
// convergence, the primal-infeasibility certificate, the stall rule, the penalty update and
// the weight of a tight row in the polish hand-over.  Scalars in, scalars out: no lane operation, no memory access, no
// barrier, no layout.  A kernel gathers its values (registers, LDS, workspace), reduces them across lanes and waves,
// and asks these functions what they mean.  Restated independently in oracle/admm_port.c and oracle/admm_ref.py;
// tests/test_check_rules.py compiles this header for the host and pins every branch.
//
// `C` is how a kernel materialises a double literal: PlainConst (the literal itself) or ScalarConst
// (acn_qp_common.hpp: a scalar register pair, opaque to the optimiser, for the kernels that run at their register limit).
#pragma once
#include <cmath>

namespace acnqp {

constexpr int kStatusPolish = 6;   // internal status: "left to the polish kernel" (never returned to a caller)

// row types of the (internally ordered) site rows
constexpr int kRowFree = 0;    // padding row: no constraint
constexpr int kRowBox = 1;     // z <= limit
constexpr int kRowSocRe = 2;   // pairs with the next register (kRowSocIm): |(re, im)| <= limit
constexpr int kRowSocIm = 3;
constexpr int kRowPeak = 4;    // z <= peak[b][t]
constexpr int kRowMax = 6;     // prox of dc * max(max_t z_t, floor) over the whole horizon (demand charge)
constexpr int kRowQuad = 5;    // prox of 1/2 lf z^2 (load flattening): z = zh rho / (rho + lf)

// Stall rule: a problem whose residual score max(pri / eps_pri, dua / eps_dua) has not improved by 10 % for
// kStallIters iterations and sits within kStallNear of its best score (i.e. on the plateau, not in the transient after
// a rho change) is finished: SOLVED_INACCURATE if it qualifies by inaccurate_ok (acn_qp_common.hpp), MAX_ITER otherwise (what it would be
// max_iter - it iterations later; the binding's second pass re-solves both kinds).  Converging problems never
// wait that long between improvements (longest wait seen on solved instances of every shape in tools/ and tests/:
// 1,240 iterations, a caltech54 x 12 LINEAR LP); the ones that do are the tangentially degenerate congested instances of DESIGN.md section 6, which
// otherwise burn max_iter iterations on a plateau and end with the same status.
constexpr double kStallGain = 0.9, kStallNear = 1.25;   // the window is acnqp_options.stall_iters (default 3000, 0 = off)
constexpr double kAdaptWiden = 8.0;   // rho adaptation band: adapt_tol (1 + adaptations / kAdaptWiden): no limit cycles

struct PlainConst { static constexpr double c(double v) { return v; } };

// ---- convergence -------------------------------------------------------------------------------------------------------
template <typename real> struct CheckTol { real eps_p, eps_d; };
template <typename real>
__host__ __device__ inline CheckTol<real> check_tolerances(double eps_abs, double eps_rel, real npri, real ndua) {
  return {(real)eps_abs + (real)eps_rel * npri, (real)eps_abs + (real)eps_rel * ndua};
}
template <typename real>
__host__ __device__ inline bool converged(real pri, real dua, const CheckTol<real>& e) { return pri <= e.eps_p && dua <= e.eps_d; }

// ---- primal infeasibility certificate (OSQP's, generalised to the sets B and C) ------------------------------------------
// v = y - y(previous check).  If A'v ~ 0 and the support function of B x C at v is negative, no point of B x C can
// satisfy A r = z: infeasible.  vn = |v|_inf, atv = |v1 + G'v2|_inf.  The gate: is v a direction worth testing, and
// with which tolerance.
template <typename real, typename C = PlainConst>
__host__ __device__ inline bool cert_gate(real vn, real atv, real qnorm, real& vtol) {
  vtol = (real)C::c(1e-4) * vn;
  return vn > (real)C::c(1e-12) * fmax((real)1, qnorm) && atv <= vtol;
}
// One site row of the ray: its share of the support function of C goes to `ssum`; `bad` is set where the row admits no
// ray in the direction of v (the support function is +inf there).  `vi` is the partner of a kRowSocRe row, `peak` the
// limit of a kRowPeak row in the lane's period (`big`: none).
__host__ __device__ inline bool cert_row_has_limit(int ty) { return ty == kRowBox || ty == kRowSocRe; }   // rows whose `lim` is read
template <typename real>
__host__ __device__ inline void cert_row_ray(int ty, real v, real vi, real lim, real peak, real big, real vtol, real& ssum, real& bad) {
  if (ty == kRowBox) { ssum += lim * fmax(v, (real)0); if (v < -vtol) bad = 1; }
  else if (ty == kRowPeak) {
    if (peak < big) ssum += peak * fmax(v, (real)0); else if (v > vtol) bad = 1;
    if (v < -vtol) bad = 1;
  } else if (ty == kRowSocRe) {
    ssum += lim * sqrt(v * v + vi * vi);
  } else if (ty == kRowSocIm) {   // counted with its kRowSocRe partner
  } else if (fabs(v) > vtol) bad = 1;   // free / prox rows admit no ray
}
// A session's support function is bounded above by phi(l) = l cap + sum_t [ub (v_t - l)+ + lb (v_t - l)-] for any
// admissible l; the kernels try l = min v, max v and 0 (clamped at 0 for inequality rows) and keep the smallest bound.
// Periods outside every window are pinned to lb (= ub): support lb * v.  The kernels own the order of the sums.
template <typename real>
__host__ __device__ inline real cert_session_candidate(real l, bool eq) { return eq ? l : fmax(l, (real)0); }
template <typename real>
__host__ __device__ inline real cert_support_term(real ub, real lb, real dv) { return ub * fmax(dv, (real)0) + lb * fmin(dv, (real)0); }
template <typename real>
__host__ __device__ inline bool cert_verdict(real bad_max, real stot, real vtol) { return bad_max == (real)0 && stot < -vtol; }

// ---- stall rule (kStallGain, kStallNear above) -----------------------------------------------------------------------------
template <typename real, typename C = PlainConst>
__host__ __device__ inline real stall_score(real pri, real dua, const CheckTol<real>& e) {
  const real tiny_ = (real)C::c(1e-300);
  return fmax(pri / fmax(e.eps_p, tiny_), dua / fmax(e.eps_d, tiny_));
}
template <typename real, typename C = PlainConst>
__host__ __device__ inline bool stall_improved(real score, real best_score) { return score < (real)C::c(kStallGain) * best_score; }
template <typename real, typename C = PlainConst>
__host__ __device__ inline bool stall_reached(int stall_iters, int it, int best_it, real score, real best_score) {
  return stall_iters > 0 && it - best_it >= stall_iters && score <= (real)C::c(kStallNear) * best_score;
}

// ---- rho adaptation: rho *= sqrt(relative primal / relative dual residual) once that ratio leaves a band that widens
// with every adaptation (no limit cycles); the new rho is clamped to [1e-6, 1e6].  (A kernel tests the band, counts the
// adaptation and rebuilds what depends on rho; the order of a check's verdicts -- done, hand-over, iteration limit or
// stall, adaptation -- is each kernel's own if-chain: sharing it cost the headline kernel a register)
template <typename real, typename C = PlainConst>
__host__ __device__ inline real rho_ratio(real pri, real dua, real npri, real ndua) {
  const real e12_ = (real)C::c(1e-12);
  const real sp = pri / fmax(npri, e12_);
  const real sd = dua / fmax(ndua, e12_);
  return sqrt(sp / fmax(sd, (real)C::c(1e-30)));
}
template <typename real>
__host__ __device__ inline bool rho_outside_band(real ratio, double adapt_tol, int n_adapt) {
  const real tol_eff = (real)adapt_tol * ((real)1 + (real)n_adapt * (real)(1.0 / kAdaptWiden));
  return ratio > tol_eff || ratio < (real)1 / tol_eff;
}
template <typename real, typename C = PlainConst>
__host__ __device__ inline real rho_clamped(real rho) { return fmin(fmax(rho, (real)C::c(1e-6)), (real)C::c(1e6)); }

// ---- polish hand-over: rows the polish's Schur system would have -- one per tight box / peak row, two per tight disc
// (normal + tangent), kRowSocIm counted with its partner; `live`: the row's period exists.  A problem whose count does
// not fit the polish's row tables is not handed over (it would come straight back) and the ADMM goes on.
template <typename real, typename C = PlainConst>
__host__ __device__ inline real polish_ytol(real qnorm) { return (real)C::c(1e-9) * fmax((real)1, qnorm); }
template <typename real>
__host__ __device__ inline real polish_row_weight(int ty, real yr, real yi, real ytol, bool live) {
  const bool disc = ty == kRowSocRe;
  const real mag = disc ? sqrt(yr * yr + yi * yi) : yr;
  const bool counts = (disc | (ty == kRowBox) | (ty == kRowPeak)) & live & (mag > ytol);
  return counts ? (disc ? (real)2 : (real)1) : (real)0;
}
template <typename real>
__host__ __device__ inline bool polish_fits(real cnt, int pol_rows) { return cnt + (real)8 <= (real)pol_rows; }

}  // namespace acnqp
