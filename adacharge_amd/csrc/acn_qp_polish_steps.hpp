// The Newton polish's steps that polish_kernel<4 | 8> (acn_qp_polish.hpp) and polish_long_kernel (acn_qp_polish_long.hpp)
// share: every phase that works on tables -- the site rows, the Schur rows, the packed blocks, the capacitance matrix --
// rather than on a thread's own variables, stated ONCE.  The tables are plain pointers: the short kernel hands in LDS, the
// long kernel its slab of global memory (and LDS for what it stages).  A function is named after the step of
// oracle/polish_ref.py (the executable specification of both kernels) it implements; the tolerances, the tie rule, the
// tangent-row rule and the noise-floor rule live here and nowhere else.
//
// Two things differ between the kernels inside these steps, and each is a policy a step takes as a template argument:
//   - where the tight site rows are kept: PolTightMask (a 32-bit mask per site row, bit t) / PolTightBytes (a byte per
//     (site row, period));
//   - how a blocking constraint is packed into the int the block-wide argmin carries: PolCode8 (8 bits for a period) /
//     PolCode12 (12 bits).
// `Ix` is the integer type a kernel indexes its (EVSE, period) tables with: int in LDS, size_t in the slab.
//
// What is NOT here, on purpose: the per-thread phases (own variables and sessions, steps 1, 4, the first half of 7, the
// variable and session halves of 8 and 10, the move, the stationarity loop of the KKT check, writing x) -- register arrays
// and bit masks, fully unrolled, in the short kernel, loops over the slab in the long one --, and steps 6a / 6b staging, 6c
// and 6e, where the long kernel's arithmetic differs.  (pol_step6_lds states 6a ... 6e on LDS tables for
// the adjoint kernel, acn_qp_vjp.hpp, which runs ONE such round: DESIGN.md 3.6i.)
//
// The first part (constants, PolishArgs, codes, the triangle index) compiles on the host: tests/host/polish_steps.cpp.
#pragma once
#include <math.h>
#include <stdint.h>

#include "acn_qp_pollds.hpp"
#include "acn_qp_polslab.hpp"

#if defined(__HIPCC__)
#define ACNQP_POL_FN __host__ __device__ inline
#else
#define ACNQP_POL_FN inline
#endif

namespace acnqp {

constexpr int kPolMaxRounds = 96;        // (kPolThreads, kPolMaxRows, kPolMaxSess: acn_qp_pollds.hpp)
constexpr double kPolTolBound = 1e-7;    // |x - bound| below which the ADMM iterate counts as "on the bound"
constexpr double kPolTolRow = 1e-9;      // relative size of a site-row multiplier that counts as non-zero
constexpr double kPolTolStep = 1e-7;     // convergence of a round: |dx|_inf <= tol max(1, |x|_inf) (1e-9 sat below the noise the
                                         // regularised solve leaves in dx on the degenerate instances: six idle rounds; the KKT check decides)
constexpr double kPolTolDual = 1e-9;     // a multiplier below -tol max(1, |q|_inf) leaves the working set
constexpr double kPolTolPrimal = 1e-9;   // accepted violation of a row, relative to max(1, limit)
constexpr double kPolRegRel = 1e-9;      // dual regularisation of the Schur system, relative to pd ...
constexpr double kPolRegDiag = 1e-12;    // ... and to the largest |R_a|^2, whichever is larger (oracle/polish_ref.py: REG_DIAG)
constexpr int kPolStallRounds = 4;       // full steps without progress that count as the noise floor of the regularised solve
constexpr double kPolTangentMin = 1e-7;  // a disc with a multiplier below tol max(1, |q|_inf) gets no curvature row

struct PolishArgs {
  int B, N, Tm, K, M, Mg, cone, has_peak;
  int max_rows;      // rows of the Schur system the row tables hold (<= kPolMaxRows)
  int blk_doubles;   // LDS doubles for the per-period blocks of the system (phase 5)
  int max_sess;      // columns of V (tight sessions with free variables) the capacitance matrix holds
  const double *G, *limits;        // acnqp_site.G [Mg][N] and limits [M] as the caller gave them (no equilibration)
  const int32_t* horizon;
  const double *lb, *ub, *q, *pdiag;
  const int32_t *s_off, *s_len;
  const double* s_cap;
  const uint8_t* s_eq;
  const double* peak;
  double *x, *y;                   // in: the ADMM iterate (schedule, site-row multipliers in the caller's units); out: the optimum
  int32_t *status, *iters;
  double *pri, *dua, *obj;
  const int32_t *list, *count;     // problems left to the polish by the solver kernel
  int32_t* queue;                  // launch counter of the work queue
  int32_t* stats;                  // [0] attempted, [1] succeeded, [2] gave up: rows, [3] pivot, [4] rounds, [5] verification
  double reg_rel;
  // -- a launch ALONGSIDE the solver launch that fills `list` (acn_qp_polclaim.hpp): entries are claimed as
  //    they are published, until the solver's `retired` count reaches `expected` problems or max_polls polls have passed
  int alongside;                   // 0: the serial launch behind the solver (the list is complete: `count` entries)
  int expected;
  const int32_t* retired;
  long long max_polls;
  int32_t* taken;                  // problems the launches alongside took (acnqp_debug_polish_alongside)
};

// blocking-constraint / release codes: kind in the top bits, then an EVSE or site row (p0), then a period or session slot
// (p1).  Ordered like (kind, p0, p1): ties of the block-wide argmin go to the smaller code.
constexpr int kPolLb = 0, kPolUb = 1, kPolSess = 2, kPolRow = 3;
struct PolCode8 {    // 8 bits for a period: horizons <= 32
  ACNQP_POL_FN static int make(int kind, int p0, int p1) { return (kind << 24) | (p0 << 8) | p1; }
  ACNQP_POL_FN static int kind(int code) { return code >> 24; }
  ACNQP_POL_FN static int p0(int code) { return (code >> 8) & 0xffff; }
  ACNQP_POL_FN static int p1(int code) { return code & 0xff; }
};
struct PolCode12 {   // 12 bits: horizons <= 288 (pol_code_long of acn_qp_polslab.hpp)
  ACNQP_POL_FN static int make(int kind, int p0, int p1) { return pol_code_long(kind, p0, p1); }
  ACNQP_POL_FN static int kind(int code) { return pol_code_long_kind(code); }
  ACNQP_POL_FN static int p0(int code) { return pol_code_long_p0(code); }
  ACNQP_POL_FN static int p1(int code) { return pol_code_long_p1(code); }
};

// row of entry p of a packed lower triangle (row r holds entries [r (r + 1) / 2, r (r + 1) / 2 + r]); its column is
// p - r (r + 1) / 2
ACNQP_POL_FN int pol_tri_row(int p) {
  int r = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
  while ((r + 1) * (r + 2) / 2 <= p) ++r;
  while (r * (r + 1) / 2 > p) --r;
  return r;
}

}  // namespace acnqp

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "acn_qp_common.hpp"

namespace acnqp {

// ---- reductions and the per-block solve -------------------------------------------------------------------------------------

// LDS traffic inside ONE wave: writes of some lanes read by others in the next step (the tiled kernel's idiom)
__device__ inline void pol_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// B_t^-1 applied in place to the rows [a0, a0 + mt) of the LDS vector `v`, by ONE wave: blk = the block's packed L D L'
// (L unscaled, pol_block_factor), dinv = 1 / D of its rows.
__device__ inline void pol_block_solve(const double* blk, const double* dinv, double* v, int mt, int lane) {
  for (int k = 0; k < mt; ++k) {          // L z = v
    const double zk = v[k] * dinv[k];
    for (int r = k + 1 + lane; r < mt; r += 64) v[r] -= blk[r * (r + 1) / 2 + k] * zk;
    pol_wave_sync();
  }
  for (int r = lane; r < mt; r += 64) v[r] *= dinv[r];
  pol_wave_sync();
  for (int k = mt - 1; k > 0; --k) {      // L' x = D^-1 z
    const double xk = v[k];
    for (int c = lane; c < k; c += 64) v[c] -= blk[k * (k + 1) / 2 + c] * dinv[c] * xk;
    pol_wave_sync();
  }
}

__device__ inline double pol_quad_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}
__device__ inline double pol_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
// block-wide max; every thread gets it (two barriers; `red` holds one double per wave)
__device__ inline double pol_block_max(double v, double* red) {
  v = pol_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
__device__ inline double pol_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
// block-wide minimum with a payload; ties go to the smaller code (deterministic).  code < 0: no candidate.
__device__ inline void pol_block_argmin(double& v, int& code, double* red) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oc = __shfl_xor(code, o);
    const bool take = oc >= 0 && (code < 0 || ov < v || (ov == v && oc < code));
    v = take ? ov : v;
    code = take ? oc : code;
  }
  int* redi = reinterpret_cast<int*>(red + 4);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = code; }
  __syncthreads();
  v = red[0]; code = redi[0];
  for (int w = 1; w < 4; ++w) {
    const double ov = red[w];
    const int oc = redi[w];
    const bool take = oc >= 0 && (code < 0 || ov < v || (ov == v && oc < code));
    v = take ? ov : v;
    code = take ? oc : code;
  }
}
// block-wide exclusive scan of one int per thread: `base` plus what the threads before this one hold, and the block's
// total in `total` (two barriers; `red` holds one int per wave)
__device__ __forceinline__ int pol_block_scan(int v, int base, int& total, double* red) {
  const int tid = threadIdx.x;
  int incl = v;
  for (int o = 1; o < 64; o <<= 1) { const int nb = __shfl_up(incl, o); incl += (tid & 63) >= o ? nb : 0; }
  int* WT = reinterpret_cast<int*>(red);
  __syncthreads();
  if ((tid & 63) == 63) WT[tid >> 6] = incl;
  __syncthreads();
  int before = base;
  for (int w = 0; w < (tid >> 6); ++w) before += WT[w];
  total = WT[0] + WT[1] + WT[2] + WT[3];
  return before + incl - v;
}

// ---- what the steps are handed ------------------------------------------------------------------------------------------------

// the site rows of problem b: row r < M is the site's row r (a disc with its pair at ABI rows r and r + M, or a box row), row
// M the peak row (ABI row Mg - 1)
struct PolSite {
  int N, Tm, M, Mg, nrow, b;
  bool soc;
  const double *limits, *peak;
  __device__ __forceinline__ int row_j(int r) const { return r < M ? r : Mg - 1; }
  __device__ __forceinline__ bool is_disc(int r) const { return soc && r < M; }
  __device__ __forceinline__ double lim(int r, int t) const { return r < M ? limits[r] : peak[(size_t)b * Tm + t]; }
};

// the rows of the Schur system: ABI row, site row (tangent rows: -1 - r), period; coefficients of the pair, residual,
// diagonal (then 1 / D of the row's block), right-hand side (then the multiplier)
struct PolRows {
  int *RJ, *RR, *RT;
  double *RC0, *RC1, *RCA, *RDG, *LAM;
  // R_a at EVSE e (a row lives on its own period's variables)
  __device__ __forceinline__ double at(const double* Gs, int N, int M, int a_, int e_) const {
    const int ja = RJ[a_];
    const double c1 = RC1[a_];
    return RC0[a_] * Gs[ja * N + e_] + (c1 != 0.0 ? c1 * Gs[(ja + M) * N + e_] : 0.0);
  }
};

// the tight site rows.  reset + fill: the first guess (every thread of the block, every (r, t) filled once); set / clear:
// ONE thread, between barriers.
struct PolTightMask {   // per site row: bit t = tight at period t (horizons <= 32)
  unsigned* w;
  __device__ __forceinline__ void reset(int nrow, int tid) const {
    for (int r = tid; r < nrow; r += kPolThreads) w[r] = 0;
    __syncthreads();
  }
  __device__ __forceinline__ void fill(int r, int t, int, bool on) const { if (on) atomicOr(&w[r], 1u << t); }
  __device__ __forceinline__ bool test(int r, int t, int) const { return (w[r] >> t) & 1u; }
  __device__ __forceinline__ void set(int r, int t, int) const { w[r] |= 1u << t; }
  __device__ __forceinline__ void clear(int r, int t, int) const { w[r] &= ~(1u << t); }
};
struct PolTightBytes {   // per (site row, period): a byte
  unsigned char* w;
  __device__ __forceinline__ void reset(int, int) const {}   // (fill writes every byte)
  __device__ __forceinline__ void fill(int r, int t, int Tm, bool on) const { w[r * Tm + t] = on ? 1 : 0; }
  __device__ __forceinline__ bool test(int r, int t, int Tm) const { return w[r * Tm + t]; }
  __device__ __forceinline__ void set(int r, int t, int Tm) const { w[r * Tm + t] = 1; }
  __device__ __forceinline__ void clear(int r, int t, int Tm) const { w[r * Tm + t] = 0; }
};

// coarse phase clock (thread 0, 100 MHz ticks summed into stats[8 + phase]): where a polish spends its time
struct PolClock {
  unsigned long long tick;
  unsigned tacc[8];
  __device__ __forceinline__ void start() {
    tick = wall_clock64();
    for (int ph = 0; ph < 8; ++ph) tacc[ph] = 0;
  }
  __device__ __forceinline__ void lap(int ph) { const unsigned long long _n = wall_clock64(); tacc[ph] += (unsigned)(_n - tick); tick = _n; }
  __device__ __forceinline__ void flush(int32_t* stats, int rounds) const {   // (thread 0)
    for (int ph = 0; ph < 8; ++ph) atomicAdd(stats + 8 + ph, (int)tacc[ph]);
    atomicAdd(stats + 6, rounds);
  }
};

// noise floor (oracle/polish_ref.py): full steps that have stopped shrinking go to the multiplier test and the KKT check
// like a converged one; the check decides, and a failure there ends the polish instead of burning the round limit
struct PolStall {
  int stall;           // full steps in a row without progress
  double best_step;
  __device__ __forceinline__ void reset() { stall = 0; best_step = 1e300; }
  __device__ __forceinline__ void update(int block, double step) {
    if (block < 0) {
      stall = step >= 0.5 * best_step ? stall + 1 : 0;
      best_step = fmin(best_step, step);
    } else {
      reset();
    }
  }
  __device__ __forceinline__ bool converged(int block, double step, double xmax) const {
    const bool floor_hit = block < 0 && stall >= kPolStallRounds && step <= 1e-3;
    return block < 0 && (step <= kPolTolStep * fmax(1.0, xmax) || floor_hit);
  }
};

// the next entry of the COMPLETE list (the serial launch behind the solver): its position, or -1 when the list is through
__device__ __forceinline__ int pol_next_listed(const PolishArgs& A, int q_round, int* q_slot) {
  const int nlist = *A.count;
  return queue_next(A.queue, nlist < A.B ? nlist : A.B, q_round, q_slot);
}

// ---- the steps --------------------------------------------------------------------------------------------------------------------

// first guess of the tight site rows from the ADMM's multipliers (the caller's barrier follows)
template <class Tight>
__device__ __forceinline__ void pol_first_guess(const PolSite& S, const Tight& RACT, const double* y, double* NU, double qn, int tid) {
  const int Tm = S.Tm, M = S.M, Mg = S.Mg, b = S.b;
  RACT.reset(S.nrow, tid);
  for (int k = tid; k < S.nrow * Tm; k += kPolThreads) {
    const int r = k / Tm, t = k - r * Tm, j = S.row_j(r);
    const double y0 = y[((size_t)b * Mg + j) * Tm + t];
    const double mag = S.is_disc(r) ? hypot(y0, y[((size_t)b * Mg + j + M) * Tm + t]) : y0;
    const double lim = S.lim(r, t);
    const bool on = mag > kPolTolRow * qn && lim < 1e299;
    NU[k] = on ? mag : 0.0;
    RACT.fill(r, t, Tm, on);
  }
}

// out[j, t] = sum_e G[j, e] v[e, t]: G x (steps 2 and the KKT check), G dx (step 7)
template <class Ix>
__device__ __forceinline__ void pol_g_times(const double* Gs, const double* v, double* out, int N, int Tm, int Mg, int tid) {
  for (int k = tid; k < Mg * Tm; k += kPolThreads) {
    const int j = k / Tm, t = k - j * Tm;
    double s = 0;
    for (int e = 0; e < N; ++e) s += Gs[j * N + e] * v[(Ix)e * Tm + t];
    out[k] = s;
  }
}

// (3) rows of the Schur system, period-major: pair k = t nrow + r of (period, site row) -> 0 / 1 / 2 rows (a tight disc: its
// normal row and, with a multiplier worth it, its tangent row); offsets by a block-wide exclusive scan.  TSTART[0 .. Tm]:
// where a period's rows start, TSTART[Tm] the rows counted (read them behind the next barrier); rows beyond `max_rows` are
// counted but not written (the caller gives up: rows).
template <class Tight>
__device__ __forceinline__ void pol_step3_rows(const PolSite& S, const Tight& RACT, const PolRows& R, const double* U, const double* NU,
                                              int* TSTART, int max_rows, double qn, double pd, double* RED, int tid) {
  const int Tm = S.Tm, M = S.M, nrow = S.nrow;
  int base = 0;
  for (int k0 = 0; k0 < nrow * Tm; k0 += kPolThreads) {
    const int k = k0 + tid;
    const bool in = k < nrow * Tm;
    const int t = in ? k / nrow : 0, r = in ? k - t * nrow : 0, j = S.row_j(r);
    int need = 0;
    double lim = 0, u0 = 0, u1 = 0, val = 0, nu = 0;
    if (in && RACT.test(r, t, Tm)) {
      lim = S.lim(r, t);
      if (S.is_disc(r)) {
        u0 = U[j * Tm + t]; u1 = U[(j + M) * Tm + t];
        val = hypot(u0, u1);
        nu = NU[r * Tm + t];
        need = val > 1e-12 ? (nu > kPolTangentMin * qn ? 2 : 1) : 0;
      } else {
        need = 1;
      }
    }
    int total;
    const int m0 = pol_block_scan(need, base, total, RED);
    if (in && r == 0) TSTART[t] = m0;
    if (need >= 1 && m0 + need <= max_rows) {
      if (S.is_disc(r)) {
        const double n0 = u0 / val, n1 = u1 / val;
        R.RJ[m0] = j; R.RR[m0] = r; R.RT[m0] = t; R.RC0[m0] = n0; R.RC1[m0] = n1; R.RCA[m0] = lim - val; R.RDG[m0] = 0.0;
        if (need == 2) {
          R.RJ[m0 + 1] = j; R.RR[m0 + 1] = -1 - r; R.RT[m0 + 1] = t; R.RC0[m0 + 1] = -n1; R.RC1[m0 + 1] = n0; R.RCA[m0 + 1] = 0.0;
          R.RDG[m0 + 1] = pd * val / nu;
        }
      } else {
        R.RJ[m0] = j; R.RR[m0] = r; R.RT[m0] = t; R.RC0[m0] = 1.0; R.RC1[m0] = 0.0; R.RCA[m0] = lim - U[j * Tm + t]; R.RDG[m0] = 0.0;
      }
    }
    base += total;
  }
  if (tid == 0) TSTART[Tm] = base;
}

// (3) session columns of V: the tight sessions with free variables, in (EVSE, slot) order (same scan); `mine`: the thread
// speaks for its EVSE's sessions (h == 0 of a quad with an EVSE).  *ncol: the columns counted (read it behind the next
// barrier); those beyond `max_sess` are counted but not written.  `more(column, slot)`: what else a kernel keeps per column.
template <class More>
__device__ __forceinline__ void pol_step3_columns(const bool (&son)[kMaxK], const double (&nfree)[kMaxK], bool mine, int i, int max_sess,
                                                  int* SI, int* SKS, double* SISQ, int* ncol, double* RED, More more) {
  int cnt = 0;
  if (mine) {
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) cnt += son[ks] ? 1 : 0;
  }
  int total;
  int pos = pol_block_scan(cnt, 0, total, RED);
  if (threadIdx.x == 0) *ncol = total;
  if (mine) {
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks)
      if (son[ks]) {
        if (pos < max_sess) { SI[pos] = i; SKS[pos] = ks; more(pos, ks); SISQ[pos] = 1.0 / sqrt(nfree[ks]); }
        ++pos;
      }
  }
}

// packed blocks of B, one per period, one after the other (thread 0; the caller's barrier follows)
__device__ __forceinline__ void pol_block_offsets(const int* TSTART, int* BOFF, int Tm) {
  int o = 0;
  for (int t = 0; t < Tm; ++t) { BOFF[t] = o; const int mt = TSTART[t + 1] - TSTART[t]; o += mt * (mt + 1) / 2; }
  BOFF[Tm] = o;
}

// (5) rhs = R v_free - pd c_A;  B = R R' + diag + reg I, BLOCK DIAGONAL by period;  C = I
// (R P R' + diag + reg I) lam = rhs with R P R' = R R' - V V', V[:, s] = R 1_s / sqrt(n_s) over the tight sessions with free
// variables: Woodbury -- lam = y + B^-1 V w, y = B^-1 rhs, (I - V' B^-1 V) w = V' y.  Per-period L D L' factors of <= 2 nrow
// rows and one of the size of the tight sessions, instead of one dense factorisation of the size of ALL tight site rows:
// the 200-row systems of the horizon-24 stragglers fit, and a round costs what its blocks cost (oracle/polish_ref.py).
// vfree: v_free (N, Tm); CS: per (i, t) -2 where the variable is not free; m rows, E doubles of blocks, nsa columns.
template <class Ix>
__device__ __forceinline__ void pol_step5(const PolRows& R, const double* Gs, const double* vfree, const signed char* CS, const int* TSTART,
                                          const int* BOFF, double* BLK, double* CAP, int N, int Tm, int M, int m, int E, int nsa, double pd,
                                          double* RED, int tid) {
  double dloc = 0;
  for (int a = tid; a < m; a += kPolThreads) {
    const int ta = R.RT[a];
    const double* g0 = Gs + R.RJ[a] * N;        // (the row's constants once, not once per EVSE: this loop and the block
    const double* g1 = g0 + M * N;              //  build below were 20 us of a 79 us round as chains of LDS reads)
    const double c0 = R.RC0[a], c1 = R.RC1[a];
    const bool two = c1 != 0.0;
    double sacc = 0, d2 = 0;
    for (int e = 0; e < N; ++e) {
      const double ra = c0 * g0[e] + (two ? c1 * g1[e] : 0.0);
      sacc += ra * vfree[(Ix)e * Tm + ta];
      d2 += CS[(Ix)e * Tm + ta] != -2 ? ra * ra : 0.0;
    }
    R.LAM[a] = sacc - pd * R.RCA[a];
    dloc = fmax(dloc, d2);
  }
  const double reg = fmax(kPolRegRel * pd, kPolRegDiag * pol_block_max(dloc, RED));
  {
    int t = 0;
    for (int p = tid; p < E; p += kPolThreads) {
      while (BOFF[t + 1] <= p) ++t;
      const int q_ = p - BOFF[t];
      const int ar = pol_tri_row(q_);
      const int cr = q_ - ar * (ar + 1) / 2;
      const int a = TSTART[t] + ar, c = TSTART[t] + cr;
      const double *ga0 = Gs + R.RJ[a] * N, *ga1 = ga0 + M * N, *gc0 = Gs + R.RJ[c] * N, *gc1 = gc0 + M * N;
      const double a0c = R.RC0[a], a1c = R.RC1[a], c0c = R.RC0[c], c1c = R.RC1[c];
      const bool atwo = a1c != 0.0, ctwo = c1c != 0.0;
      double sacc = 0;
      for (int e = 0; e < N; ++e) {
        const double ra = a0c * ga0[e] + (atwo ? a1c * ga1[e] : 0.0);
        const double rc = c0c * gc0[e] + (ctwo ? c1c * gc1[e] : 0.0);
        sacc += CS[(Ix)e * Tm + t] != -2 ? ra * rc : 0.0;
      }
      BLK[p] = sacc + (a == c ? R.RDG[a] + reg : 0.0);
    }
  }
  for (int p = tid; p < nsa * (nsa + 1) / 2; p += kPolThreads) CAP[p] = 0.0;
  __syncthreads();
  for (int c = tid; c < nsa; c += kPolThreads) CAP[c * (c + 1) / 2 + c] = 1.0;
}

// (6a) L D L' of one packed block of mt rows in place, by ONE wave (unit lower L stored unscaled).  False: a pivot is not
// positive (wave-uniform).
__device__ __forceinline__ bool pol_block_factor(double* blk, int mt, int lane) {
  bool bad = false;
  for (int k = 0; k < mt && !bad; ++k) {
    const double piv = blk[k * (k + 1) / 2 + k];
    if (!(piv > 0.0)) { bad = true; break; }   // (wave-uniform)
    const double pinv = 1.0 / piv;
    for (int rr = k + 1 + (lane >> 3); rr < mt; rr += 8) {
      const double lr = blk[rr * (rr + 1) / 2 + k] * pinv;
      for (int c = k + 1 + (lane & 7); c <= rr; c += 8) blk[rr * (rr + 1) / 2 + c] -= lr * blk[c * (c + 1) / 2 + k];
    }
    pol_wave_sync();
  }
  return !bad;
}

// (6d) C = L D L' (packed, one barrier per column), C w = V' y: ZV holds V' y on entry and w on return; DI: nsa doubles of
// room for 1 / D.  False: a pivot is not positive (block-uniform: every thread reads the same entry).
__device__ __forceinline__ bool pol_step6d(double* CAP, double* ZV, double* DI, int nsa, int tid) {
  bool bad_pivot = false;
  for (int k = 0; k < nsa; ++k) {
    __syncthreads();
    const double piv = CAP[k * (k + 1) / 2 + k];
    if (!(piv > 0.0)) { bad_pivot = true; break; }
    const double pinv = 1.0 / piv;
    for (int rr = k + 1 + (tid >> 4); rr < nsa; rr += 16) {
      const double lr = CAP[rr * (rr + 1) / 2 + k] * pinv;
      double* row = CAP + rr * (rr + 1) / 2;
      for (int c = k + 1 + (tid & 15); c <= rr; c += 16) row[c] -= lr * CAP[c * (c + 1) / 2 + k];
    }
  }
  if (bad_pivot) return false;
  __syncthreads();
  for (int k = tid; k < nsa; k += kPolThreads) DI[k] = 1.0 / CAP[k * (k + 1) / 2 + k];
  __syncthreads();
  double acc = tid < nsa ? ZV[tid] : 0.0;   // forward: L z = V' y (thread r owns z_r)
  for (int k = 0; k < nsa; ++k) {
    if (tid == k) ZV[k] = acc;
    __syncthreads();
    if (tid > k && tid < nsa) acc -= CAP[tid * (tid + 1) / 2 + k] * DI[k] * ZV[k];
  }
  __syncthreads();
  acc = tid < nsa ? ZV[tid] * DI[tid] : 0.0;   // backward: L' w = D^-1 z
  const double dme = tid < nsa ? DI[tid] : 0.0;
  for (int k = nsa - 1; k >= 0; --k) {
    if (tid == k) ZV[k] = acc;
    __syncthreads();
    if (tid < k) acc -= CAP[k * (k + 1) / 2 + tid] * dme * ZV[k];
  }
  __syncthreads();
  return true;
}

// (6a) ... (6e) on LDS tables, phase for phase as polish_kernel<4 | 8> writes them out between its phase clocks, for a kernel
// that has none (vjp_kernel, acn_qp_vjp.hpp): the blocks' L D L' (a wave per block), y = B^-1 rhs, the capacitance matrix
// block by block, C w = V' y, lam = y + B^-1 V w.  In: LAM = rhs, BLK / CAP as pol_step5 left them.  Out: LAM = lam, RDG =
// 1 / D of the blocks; RCA, ZB and ZV are scratch.  `bad`: an int of LDS the caller has zeroed.  False: a pivot is not
// positive (block-uniform).  Ends behind a barrier.
__device__ __forceinline__ bool pol_step6_lds(const PolRows& R, const double* Gs, const signed char* CS, const int* TSTART, const int* BOFF,
                                              double* BLK, double* CAP, double* ZB, double* ZV, const double* SISQ, const int* SI, const int* SKS,
                                              int* bad, int N, int Tm, int M, int m, int nsa, int MS, int tid) {
  const int wave_ = tid >> 6, lane_ = tid & 63;
  // (6a)
  for (int t = wave_; t < Tm; t += 4) {
    const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
    double* blk = BLK + BOFF[t];
    if (!pol_block_factor(blk, mt, lane_)) { if (lane_ == 0) *bad = 1; continue; }
    for (int k = lane_; k < mt; k += 64) R.RDG[a0 + k] = 1.0 / blk[k * (k + 1) / 2 + k];
  }
  __syncthreads();
  if (*bad) return false;
  // (6b)
  for (int t = wave_; t < Tm; t += 4) {
    const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
    if (mt > 0) pol_block_solve(BLK + BOFF[t], R.RDG + a0, R.LAM + a0, mt, lane_);
  }
  __syncthreads();
  // (6c)
  for (int c = tid; c < nsa; c += kPolThreads) {
    const int ic = SI[c], ks = SKS[c];
    double z = 0;
    for (int t = 0; t < Tm; ++t)
      if (CS[ic * Tm + t] == ks)
        for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) z += R.at(Gs, N, M, a, ic) * R.LAM[a];
    ZV[c] = z * SISQ[c];
  }
  for (int t = 0; t < Tm; ++t) {
    const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
    if (mt == 0) continue;   // (block-uniform)
    const double* blk = BLK + BOFF[t];
    for (int idx = tid; idx < mt * nsa; idx += kPolThreads) {
      const int k = idx / nsa, c = idx - k * nsa;
      const int ic = SI[c];
      ZB[k * MS + c] = CS[ic * Tm + t] == SKS[c] ? R.at(Gs, N, M, a0 + k, ic) * SISQ[c] : 0.0;
    }
    __syncthreads();
    for (int c = tid; c < nsa; c += kPolThreads) {
      if (CS[SI[c] * Tm + t] != SKS[c]) continue;
      for (int k = 0; k < mt; ++k) {
        const double zk = ZB[k * MS + c] * R.RDG[a0 + k];
        for (int r = k + 1; r < mt; ++r) ZB[r * MS + c] -= blk[r * (r + 1) / 2 + k] * zk;
      }
    }
    __syncthreads();
    for (int p = tid; p < nsa * (nsa + 1) / 2; p += kPolThreads) {
      const int c = pol_tri_row(p);
      const int c2 = p - c * (c + 1) / 2;
      if (CS[SI[c] * Tm + t] != SKS[c] || CS[SI[c2] * Tm + t] != SKS[c2]) continue;
      double sacc = 0;
      for (int k = 0; k < mt; ++k) sacc += ZB[k * MS + c] * R.RDG[a0 + k] * ZB[k * MS + c2];
      CAP[p] -= sacc;
    }
    __syncthreads();
  }
  // (6d) (1 / D of C goes into the Z buffer, free now)
  if (!pol_step6d(CAP, ZV, ZB, nsa, tid)) return false;
  // (6e)
  for (int a = tid; a < m; a += kPolThreads) {
    const int ta = R.RT[a];
    double sacc = 0;
    for (int c = 0; c < nsa; ++c) {
      const int ic = SI[c];
      if (CS[ic * Tm + ta] == SKS[c]) sacc += R.at(Gs, N, M, a, ic) * SISQ[c] * ZV[c];
    }
    R.RCA[a] = sacc;
  }
  __syncthreads();
  for (int t = wave_; t < Tm; t += 4) {
    const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
    if (mt > 0) pol_block_solve(BLK + BOFF[t], R.RDG + a0, R.RCA + a0, mt, lane_);
  }
  __syncthreads();
  for (int a = tid; a < m; a += kPolThreads) R.LAM[a] += R.RCA[a];
  __syncthreads();
  return true;
}

// (8) ratio test, the site rows outside the working set
template <class Tight, class Code>
__device__ __forceinline__ void pol_step8_rows(const PolSite& S, const Tight& RACT, const double* U, const double* DU, double& alpha, int& block,
                                               int tid) {
  const int Tm = S.Tm, M = S.M;
  for (int k = tid; k < S.nrow * Tm; k += kPolThreads) {
    const int r = k / Tm, t = k - r * Tm, j = S.row_j(r);
    if (RACT.test(r, t, Tm)) continue;
    const double lim = S.lim(r, t);
    if (!(lim < 1e299)) continue;
    if (S.is_disc(r)) {
      const double u0 = U[j * Tm + t], u1 = U[(j + M) * Tm + t], d0 = DU[j * Tm + t], d1 = DU[(j + M) * Tm + t];
      const double aa = d0 * d0 + d1 * d1, bb = 2.0 * (u0 * d0 + u1 * d1), cc = u0 * u0 + u1 * u1 - lim * lim;
      if (aa > 1e-28 && (bb > 0 || cc > 0)) {
        const double dsc = bb * bb - 4.0 * aa * cc;
        if (dsc >= 0) {
          const double a_ = fmax((-bb + sqrt(dsc)) / (2.0 * aa), 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolRow, r, t); }
        }
      }
    } else {
      const double du = DU[j * Tm + t];
      if (du > 1e-14) {
        const double a_ = fmax((lim - U[j * Tm + t]) / du, 0.0);
        if (a_ < alpha) { alpha = a_; block = Code::make(kPolRow, r, t); }
      }
    }
  }
}

// (9) the new multipliers of the site rows: those of the NORMAL rows of the system, zero elsewhere
__device__ __forceinline__ void pol_step9_multipliers(const PolRows& R, double* NU, int m, int nrow, int Tm, int tid) {
  for (int k = tid; k < nrow * Tm; k += kPolThreads) NU[k] = 0.0;
  __syncthreads();
  for (int a = tid; a < m; a += kPolThreads)
    if (R.RR[a] >= 0) NU[R.RR[a] * Tm + R.RT[a]] = R.LAM[a];
}

// (10) the most negative multiplier, the site rows inside the working set
template <class Tight, class Code>
__device__ __forceinline__ void pol_step10_rows(const Tight& RACT, const double* NU, int nrow, int Tm, double& worst, int& who, int tid) {
  for (int k = tid; k < nrow * Tm; k += kPolThreads) {
    const int r = k / Tm, t = k - r * Tm;
    if (RACT.test(r, t, Tm) && NU[k] < worst) { worst = NU[k]; who = Code::make(kPolRow, r, t); }
  }
}

// KKT check: primal violation of the site rows at the final x (U = G x), relative to max(1, limit)
__device__ __forceinline__ void pol_kkt_rows(const PolSite& S, const double* U, double& pvl, int tid) {
  const int Tm = S.Tm, M = S.M;
  for (int k = tid; k < S.nrow * Tm; k += kPolThreads) {
    const int r = k / Tm, t = k - r * Tm, j = S.row_j(r);
    const double lim = S.lim(r, t);
    if (!(lim < 1e299)) continue;
    const double val = S.is_disc(r) ? hypot(U[j * Tm + t], U[(j + M) * Tm + t]) : U[j * Tm + t];
    pvl = fmax(pvl, (val - lim) / fmax(1.0, lim));
  }
}

// results of problem b, after the kernel has written x of a success: `ol` = the thread's part of the objective.  Success:
// the site-row multipliers in the caller's units (a disc's pair: nu times its outward normal, at the final x: U is
// current), status, iters, residuals, objective.  Failure: the rounds and the reason `why` (index into stats).
__device__ __forceinline__ void pol_results(const PolishArgs& A, const PolSite& S, const double* NU, const double* U, bool success, double ol,
                                            int rounds, int why, double prim_out, double stat_out, double* RED, int tid) {
  const int Tm = S.Tm, M = S.M, Mg = S.Mg, b = S.b;
  if (success) {
    const double o = pol_block_sum(ol, RED);
    for (int k = tid; k < Mg * Tm; k += kPolThreads) A.y[(size_t)b * Mg * Tm + k] = 0.0;
    __syncthreads();
    for (int k = tid; k < S.nrow * Tm; k += kPolThreads) {
      const int r = k / Tm, t = k - r * Tm, j = S.row_j(r);
      const double nu = NU[k];
      if (nu == 0.0) continue;
      if (S.is_disc(r)) {
        const double u0 = U[j * Tm + t], u1 = U[(j + M) * Tm + t], val = hypot(u0, u1);
        if (val > 0) {
          A.y[((size_t)b * Mg + j) * Tm + t] = nu * u0 / val;
          A.y[((size_t)b * Mg + j + M) * Tm + t] = nu * u1 / val;
        }
      } else {
        A.y[((size_t)b * Mg + j) * Tm + t] = nu;
      }
    }
    if (tid == 0) {
      A.status[b] = 1;
      A.iters[b] += rounds;
      A.pri[b] = fmax(prim_out, 0.0);
      A.dua[b] = stat_out;
      A.obj[b] = o;
      atomicAdd(A.stats + 1, 1);
    }
  } else if (tid == 0) {
    A.iters[b] += rounds;
    atomicAdd(A.stats + why, 1);
  }
  __syncthreads();
}

}  // namespace acnqp
#endif  // __HIPCC__
