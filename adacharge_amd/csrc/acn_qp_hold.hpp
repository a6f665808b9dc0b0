// Select and hold (acnqp_select_device / acnqp_hold_device, include/acn_qp.h): the two links that let a closed loop solve
// only the scenarios that have an event.  Which scenario resolves at which step follows from arrivals, departures and
// max_recompute, all known before the run (rollout.FleetTable.resolve_rows), so the host knows the size of every step's
// solve and never has to read an answer:
//   select  the problems idx[0:m] of the resident state, gathered into a dense batch of m problems (rules S1, S2)
//   hold    the dense answers scattered back into the full batch; every other scenario keeps the schedule it holds -- the
//           advance's shifted warm_x', clipped into the state's bounds -- and the status of the solve it came from
//           (rules H1 - H3)
// The mask never depends on the answers: a scenario whose last solve was not accepted keeps that status, and the advance
// delivers nothing for it (its rule 1) until its next scheduled solve.  That is what keeps the loop free of host
// synchronisation.
//
// tests/hold_spec.py states the rules in plain loops; the kernels are held to it BIT FOR BIT.  That is possible because
// every element is a copy, a constant or the outcome of two comparisons.
//
// One workgroup per OUTPUT problem, its size chosen by the shape only (advance_threads' rule): ONE wavefront for N <= 64,
// four beyond.  Consecutive threads take consecutive elements of the N*Tm arrays: every access is coalesced, every store
// is a plain store of at most 64 bits.  Every index that comes from caller data is range-checked before use.  No atomics,
// no barriers; every output element is written whatever the input; a problem's output does not depend on where it stands.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace acnqp {

constexpr int kSelectBadIndex = 1;   // flags[j] of select (ACNQP_SELECT_BAD_INDEX)
constexpr int kHoldBadRow = 1;       // flags[b] of hold (ACNQP_HOLD_BAD_ROW)
constexpr double kHoldInf = __builtin_huge_val();

struct SelectArgs {
  int B, m, N, Tm, K, Mg;
  const int32_t* idx;                              // [m]
  // the state: B problems (an optional array may be nullptr, then so is its output)
  const int32_t* horizon;
  const double *lb, *ub, *q, *pdiag;
  const int32_t *s_off, *s_len;
  const double* s_cap;
  const uint8_t* s_eq;
  const double *peak, *lf, *dc, *dfloor, *wx, *wy;
  // the dense batch: m problems
  int32_t* o_horizon;
  double *o_lb, *o_ub, *o_q, *o_pdiag;
  int32_t *o_off, *o_len;
  double* o_cap;
  uint8_t* o_eq;
  double *o_peak, *o_lf, *o_dc, *o_dfloor, *o_wx, *o_wy;
  int32_t* flags;                                  // [m]
};

struct HoldArgs {
  int B, m, N, Tm, Mg;
  const int32_t* pos;                              // [B]
  const double *rx, *ry;                           // [m][N][Tm], [m][Mg][Tm] or nullptr
  const int32_t *rstatus, *riters;                 // [m]
  const double *held_x, *held_y;                   // [B][N][Tm], [B][Mg][Tm] or nullptr
  const int32_t* prev_status;                      // [B]
  const double *lb, *ub;                           // [B][N][Tm]
  double *x, *y;                                   // y: nullptr = not wanted
  int32_t *status, *iters;
  uint8_t* solved;
  int32_t* flags;                                  // [B]
};

inline int hold_threads(int N) { return N <= 64 ? 64 : 256; }   // (advance_threads' rule)

// The order of two doubles (no NaN) read off their bit patterns: hold_key(a) < hold_key(b) iff a < b, and -0.0 and +0.0
// get the same key, as the floating-point comparison has it.  Rule H2 compares and then COPIES one of its three inputs:
// done on doubles, the compiler turns the pair into v_min_f64 / v_max_f64, which order the zeros (max(-0.0, +0.0) is
// +0.0 where the rule keeps -0.0).  On the bit patterns the element that comes out is an input, bit for bit.
__host__ __device__ inline long long hold_key(long long bits) {
  const long long k = bits ^ ((bits >> 63) & 0x7fffffffffffffffLL);   // negative numbers: larger magnitude, smaller key
  return k - (k >> 63);                                                // ... moved up by one, so that -0.0 meets +0.0 at 0
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void select_kernel(const SelectArgs A) {
  const int gt = (int)threadIdx.x, j = (int)blockIdx.x;
  const int b = A.idx[j];
  const bool ok = b >= 0 && b < A.B;               // S1, else S2: nothing of the state is read
  const int n = A.N * A.Tm, ns = A.K * A.N, ny = A.Mg * A.Tm;   // (N <= 1024, Tm, K <= 4096: 32-bit inside a problem)
  const size_t src = ok ? (size_t)b : 0, dst = (size_t)j;
  {
    const double *lb = A.lb + src * n, *ub = A.ub + src * n, *q = A.q + src * n;
    double *ol = A.o_lb + dst * n, *ou = A.o_ub + dst * n, *oq = A.o_q + dst * n;
    for (int k = gt; k < n; k += THREADS) {
      ol[k] = ok ? lb[k] : 0.0;
      ou[k] = ok ? ub[k] : 0.0;
      oq[k] = ok ? q[k] : 0.0;
    }
    if (A.o_wx) {
      const double* w = A.wx + src * n;
      double* ow = A.o_wx + dst * n;
      for (int k = gt; k < n; k += THREADS) ow[k] = ok ? w[k] : 0.0;
    }
    if (A.o_wy) {
      const double* w = A.wy + src * ny;
      double* ow = A.o_wy + dst * ny;
      for (int k = gt; k < ny; k += THREADS) ow[k] = ok ? w[k] : 0.0;
    }
  }
  for (int s = gt; s < ns; s += THREADS) {
    A.o_off[dst * ns + s] = ok ? A.s_off[src * ns + s] : 0;
    A.o_len[dst * ns + s] = ok ? A.s_len[src * ns + s] : 0;
    A.o_cap[dst * ns + s] = ok ? A.s_cap[src * ns + s] : 0.0;
  }
  if (A.o_peak)
    for (int t = gt; t < A.Tm; t += THREADS) A.o_peak[dst * A.Tm + t] = ok ? A.peak[src * A.Tm + t] : kHoldInf;
  if (gt == 0) {
    A.o_horizon[j] = ok ? A.horizon[b] : 1;
    A.o_pdiag[j] = ok ? A.pdiag[b] : 0.0;
    A.o_eq[j] = ok ? A.s_eq[b] : (uint8_t)0;
    if (A.o_lf) A.o_lf[j] = ok ? A.lf[b] : 0.0;
    if (A.o_dc) A.o_dc[j] = ok ? A.dc[b] : 0.0;
    if (A.o_dfloor) A.o_dfloor[j] = ok ? A.dfloor[b] : 0.0;
    A.flags[j] = ok ? 0 : kSelectBadIndex;
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void hold_kernel(const HoldArgs A) {
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int j = A.pos[b];
  const bool taken = j >= 0 && j < A.m;            // H1, else H2: nothing of the dense results is read
  const int n = A.N * A.Tm, ny = A.Mg * A.Tm;
  const size_t pb = (size_t)b * n;
  double* x = A.x + pb;
  if (taken) {
    const double* rx = A.rx + (size_t)j * n;
    for (int k = gt; k < n; k += THREADS) x[k] = rx[k];
  } else {
    const long long* hx = reinterpret_cast<const long long*>(A.held_x + pb);
    const long long* lb = reinterpret_cast<const long long*>(A.lb + pb);
    const long long* ub = reinterpret_cast<const long long*>(A.ub + pb);
    long long* xb = reinterpret_cast<long long*>(x);
    for (int k = gt; k < n; k += THREADS) {
      long long v = hx[k];
      const long long hi = ub[k], lo = lb[k];
      if (hold_key(v) > hold_key(hi)) v = hi;      // v > ub, then v < lb: comparisons only, in this order
      if (hold_key(v) < hold_key(lo)) v = lo;
      xb[k] = v;
    }
  }
  if (A.y) {
    const double* sy = taken ? A.ry + (size_t)j * ny : A.held_y + (size_t)b * ny;
    double* y = A.y + (size_t)b * ny;
    for (int k = gt; k < ny; k += THREADS) y[k] = sy[k];
  }
  if (gt == 0) {
    A.status[b] = taken ? A.rstatus[j] : A.prev_status[b];
    A.iters[b] = taken ? A.riters[j] : 0;
    A.solved[b] = taken ? (uint8_t)1 : (uint8_t)0;
    A.flags[b] = taken || j == -1 ? 0 : kHoldBadRow;   // H3
  }
}

hipError_t launch_select(const SelectArgs& a, hipStream_t st);
hipError_t launch_hold(const HoldArgs& a, hipStream_t st);

}  // namespace acnqp
