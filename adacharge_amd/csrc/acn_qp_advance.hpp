// Time passes (acnqp_advance_device / acnqp_advance_host, include/acn_qp.h): the problems a batch just solved and the
// pilots just applied in, the next control period's problems out -- the fourth link of a closed MPC loop (solve, pilots,
// duals, advance), so that a batch of scenario simulations keeps its state in HBM from the first period to the last.
// What the reference's users do on the host every period: integrate the delivered energy, drop the sessions that are
// done, admit the arrivals, rebuild bounds, energy rows and the objective for the new horizon (aco.py:45-124, 200-245).
//
// tests/advance_spec.py states the ten rules of include/acn_qp.h in plain loops; the kernel is held to it BIT FOR BIT.
// That is possible because everything is a copy, an integer operation or a comparison, except
//   * one subtraction per served slot, cap' = cap - a_i, and
//   * one sum per problem, sum_i a_i in increasing i inside ONE thread, then one product and one comparison
// (contraction is switched off inside the kernel).
//
// One workgroup per problem, its size chosen by the shape only (advance_threads): ONE wavefront for N <= 64, four
// beyond.  The output never aliases the input (the entry points refuse it): the phases of a problem are ordered by
// workgroup barriers and a later phase overwrites what an earlier one wrote --
//   1  bounds and warm start shifted by one period (streamed by all threads); the applied pilots staged in LDS
//   2  one thread per slot: the slot's new (off, len, cap); a retired slot zeroes its window of the shifted bounds
//   3  one thread per EVSE: the problem's arrival records in record order (serial per EVSE), checked, then admitted
//   4  the new horizon (a workgroup maximum over the live slots), then the linear cost of that horizon, the scalars,
//      the peak row, the demand-charge floor and the flags
// Every index that comes from caller data is range-checked before use; a bad record raises a flag and is skipped.  No
// atomics; every output element is written whatever the input; a problem gives the same bits alone and at any position of
// any batch.
//
// With a clock cost (acnqp_advance_priced_device / _host, rule 6b; spec tests/advance_priced_spec.py) the CLOCK
// instantiations add coef * (weight[i] * series[b][step + 1 + t]) to q' inside the new horizon: two products and one sum
// per entry, each rounded once -- the builder's q of an objective whose last component is coef * tou_energy_cost.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace acnqp {

constexpr int kAdvanceRefused = 1, kAdvanceNoRow = 2, kAdvanceBadSlot = 4;   // bits of flags[b]
constexpr int kAdvSolved = 1, kAdvSolvedInaccurate = 5;                       // ACNQP_STATUS_SOLVED, _SOLVED_INACCURATE

struct AdvanceArgs {
  int B, N, Tm, K, Mg;
  // the current problems and what happened to them
  const double *lb, *ub;                   // [B][N][Tm]
  const int32_t *s_off, *s_len;            // [B][K][N]
  const double* s_cap;                     // [B][K][N]
  const double* dfloor;                    // [B] or nullptr
  const double* applied;                   // [B][N]
  const int32_t* status;                   // [B] or nullptr
  const double *x, *y;                     // [B][N][Tm], [B][Mg][Tm]: warm outputs only
  // the plan
  int H, step, P, A, R;                    // horizons of q_table, period just completed, peak_series length, arrival records, rate entries
  const double* q_table;                   // [H][N][Tm]
  const double* h_scal;                    // [H][3] pdiag, lf, dc
  const int32_t* h_row;                    // [Tm + 1]
  double done_tol, kw_per_amp;
  double warm_gain;                        // != 0: warm_x' of a session admitted in this step is -warm_gain q' on its window
  const double* peak_series;               // [B][P] or nullptr
  const int32_t* a_seg;                    // [B + 1]
  const int32_t *a_evse, *a_slot, *a_len;  // [A]
  const double* a_cap;                     // [A]
  const int32_t* a_rate_seg;               // [A + 1]
  const double *a_min, *a_max;             // [R]
  // the next problems
  int32_t* n_horizon;
  double *n_lb, *n_ub, *n_q;
  double *n_pdiag, *n_lf, *n_dc, *n_dfloor;   // n_lf, n_dc, n_dfloor may be nullptr
  int32_t *n_off, *n_len;
  double* n_cap;
  double* n_peak;                          // [B][Tm] or nullptr
  double *n_wx, *n_wy;                     // or nullptr
  int32_t* flags;                          // [B]
  // the clock cost (rule 6b), read by the CLOCK instantiations only
  int c_P = 0;                             // series length
  double c_coef = 0.0;
  const double* c_weight = nullptr;        // [N]
  const double* c_series = nullptr;        // [B][c_P]
};

inline int advance_threads(int N) { return N <= 64 ? 64 : 256; }
inline size_t advance_lds(int N) { return ((size_t)N * 12 + 15) & ~(size_t)15; }

constexpr double kAdvanceInf = __builtin_huge_val();

// CLOCK: the variant with rule 6b, q' = q_table[row] + c_coef * (c_weight[i] * c_series[b][step + 1 + t]) for t < horizon'
// (three operations, each rounded once), and rule 9 on that q'.  The plain variant reads none of the c_ fields.
template <int THREADS, bool CLOCK = false>
__global__ __launch_bounds__(THREADS) void advance_kernel(const AdvanceArgs A) {
#pragma clang fp contract(off)   // every operation of this kernel is rounded once (tests/advance_spec.py)
  extern __shared__ __attribute__((aligned(16))) char advance_lds_raw[];
  __shared__ int red_max[THREADS], red_or[THREADS];
  double* ap = reinterpret_cast<double*>(advance_lds_raw);   // [N] what was delivered: the applied pilots, or zeros
  int* fresh = reinterpret_cast<int*>(ap + A.N);             // [N] length of the session admitted in this step, or 0
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int N = A.N, Tm = A.Tm, K = A.K;
  const int n = N * Tm;   // (N <= 1024, Tm <= 4096: 32-bit index arithmetic inside a problem)
  const size_t pb = (size_t)b * n, sb = (size_t)b * K * N;
  int flag = 0;

  // ---- 1: rule 1 (what was delivered), rules 3 and 9 (the shift) -------------------------------------------------------
  const int st = A.status ? A.status[b] : kAdvSolved;
  const bool served = st == kAdvSolved || st == kAdvSolvedInaccurate;
  for (int i = gt; i < N; i += THREADS) {
    ap[i] = served ? A.applied[(size_t)b * N + i] : 0.0;
    fresh[i] = 0;
  }
  {
    const double *lb = A.lb + pb, *ub = A.ub + pb;
    double *nl = A.n_lb + pb, *nu = A.n_ub + pb;
    for (int k = gt; k < n; k += THREADS) {
      const int t = k % Tm;
      const bool in = t + 1 < Tm;
      nl[k] = in ? lb[k + 1] : 0.0;
      nu[k] = in ? ub[k + 1] : 0.0;
    }
    if (A.n_wx) {
      const double* x = A.x + pb;
      double* wx = A.n_wx + pb;
      for (int k = gt; k < n; k += THREADS) wx[k] = (k % Tm) + 1 < Tm ? x[k + 1] : 0.0;
    }
    if (A.n_wy) {
      const int m = A.Mg * Tm;
      const double* y = A.y + (size_t)b * m;
      double* wy = A.n_wy + (size_t)b * m;
      for (int k = gt; k < m; k += THREADS) wy[k] = (k % Tm) + 1 < Tm ? y[k + 1] : 0.0;
    }
  }
  __syncthreads();

  // ---- 2: rule 2, one thread per slot; a retired slot zeroes its window of the shifted bounds ---------------------------
  for (int s = gt; s < K * N; s += THREADS) {
    const int i = s % N;
    int off = A.s_off[sb + s], len = A.s_len[sb + s];
    double cap = A.s_cap[sb + s];
    if (len > 0) {
      bool retired = false;
      if (off < 0 || off >= Tm || len > Tm - off) {   // not a window of this horizon: dropped, never dereferenced
        flag |= kAdvanceBadSlot;
        off = 0; len = 0;
        retired = true;
      } else {
        if (off > 0) {
          off -= 1;
        } else {
          len -= 1;
          cap = cap - ap[i];
          if (cap < 0.0) cap = 0.0;
        }
        retired = len == 0 || cap <= A.done_tol;
      }
      if (retired) {
        double *nl = A.n_lb + pb + (size_t)i * Tm, *nu = A.n_ub + pb + (size_t)i * Tm;
        for (int t = off; t < off + len; ++t) { nl[t] = 0.0; nu[t] = 0.0; }
        off = 0; len = 0; cap = 0.0;
      }
    } else {
      off = 0; len = 0; cap = 0.0;
    }
    A.n_off[sb + s] = off;
    A.n_len[sb + s] = len;
    A.n_cap[sb + s] = cap;
  }
  __syncthreads();

  // ---- 3: rule 4, one thread per EVSE walks the problem's arrival records in record order --------------------------------
  {
    int a0 = A.a_seg ? A.a_seg[b] : 0, a1 = A.a_seg ? A.a_seg[b + 1] : 0;
    a0 = a0 < 0 ? 0 : a0;
    a1 = a1 > A.A ? A.A : a1;
    for (int i = gt; i < (a1 > a0 ? N : 0); i += THREADS) {
      double *nl = A.n_lb + pb + (size_t)i * Tm, *nu = A.n_ub + pb + (size_t)i * Tm;
      for (int r = a0; r < a1; ++r) {
        const int e = A.a_evse[r];
        if (e != i) {
          if (i == 0 && (e < 0 || e >= N)) flag |= kAdvanceRefused;   // (reported once, by the thread of EVSE 0)
          continue;
        }
        const int k = A.a_slot[r], len = A.a_len[r];
        const int r0 = A.a_rate_seg[r];
        bool ok = k >= 0 && k < K && len >= 1 && len <= Tm && r0 >= 0 && r0 <= A.R - len;
        if (ok) ok = A.n_len[sb + (size_t)k * N + i] == 0;                   // its slot is free
        for (int kk = 0; ok && kk < K; ++kk) {                              // [0, len) meets no live window of the EVSE
          const size_t s = sb + (size_t)kk * N + i;
          if (A.n_len[s] > 0 && A.n_off[s] < len) ok = false;
        }
        if (!ok) { flag |= kAdvanceRefused; continue; }
        const size_t s = sb + (size_t)k * N + i;
        A.n_off[s] = 0;
        A.n_len[s] = len;
        A.n_cap[s] = A.a_cap[r];
        fresh[i] = len;   // (two windows that start now meet: an EVSE admits one session per step)
        for (int t = 0; t < len; ++t) {
          const double lo = A.a_min[r0 + t], hi = A.a_max[r0 + t];
          nl[t] = lo;
          nu[t] = hi < lo ? lo : hi;   // aco.py:75
        }
      }
    }
  }
  __syncthreads();

  // ---- 4: rules 5-8 and 10 -------------------------------------------------------------------------------------------
  int hz = 1;
  for (int s = gt; s < K * N; s += THREADS) {
    const int len = A.n_len[sb + s];
    if (len > 0) { const int e = A.n_off[sb + s] + len; hz = e > hz ? e : hz; }
  }
  red_max[gt] = hz;
  red_or[gt] = flag;
  __syncthreads();
  for (int o = THREADS / 2; o > 0; o >>= 1) {
    if (gt < o) {
      red_max[gt] = red_max[gt + o] > red_max[gt] ? red_max[gt + o] : red_max[gt];
      red_or[gt] |= red_or[gt + o];
    }
    __syncthreads();
  }
  hz = red_max[0];       // 1 <= hz <= Tm: every live slot was checked against Tm
  flag = red_or[0];
  int row = A.h_row[hz];
  if (row < 0 || row >= A.H) { row = -1; flag |= kAdvanceNoRow; }
  if constexpr (CLOCK) {   // rules 6, 6b and 9: one thread writes q'[k] and, for a session admitted now, warm_x'[k] from it
    const double* q = row >= 0 ? A.q_table + (size_t)row * n : nullptr;
    const double* cs = A.c_series + (size_t)b * A.c_P + (A.step + 1);   // (t < hz <= Tm: inside the entry's series_len check)
    const bool start = A.n_wx && A.warm_gain != 0.0;
    const double g = -A.warm_gain;
    double* nq = A.n_q + pb;
    for (int k = gt; k < n; k += THREADS) {
      const int i = k / Tm, t = k % Tm;
      double v = 0.0;
      if (q) {
        v = q[k];
        if (t < hz) v = v + A.c_coef * (A.c_weight[i] * cs[t]);
      }
      nq[k] = v;
      if (start && t < fresh[i]) A.n_wx[pb + k] = g * v;
    }
  } else {
    {
      double* nq = A.n_q + pb;
      if (row >= 0) {
        const double* q = A.q_table + (size_t)row * n;
        for (int k = gt; k < n; k += THREADS) nq[k] = q[k];
      } else {
        for (int k = gt; k < n; k += THREADS) nq[k] = 0.0;
      }
    }
    if (A.n_wx && A.warm_gain != 0.0) {   // rule 9: a session admitted now starts where a cold solve would start it
      const double* q = row >= 0 ? A.q_table + (size_t)row * n : nullptr;
      double* wx = A.n_wx + pb;
      const double g = -A.warm_gain;
      for (int k = gt; k < n; k += THREADS)
        if (k % Tm < fresh[k / Tm]) wx[k] = g * (q ? q[k] : 0.0);
    }
  }
  if (A.n_peak) {
    const double* ps = A.peak_series ? A.peak_series + (size_t)b * A.P + (A.step + 1) : nullptr;
    for (int t = gt; t < Tm; t += THREADS) A.n_peak[(size_t)b * Tm + t] = ps && t < hz ? ps[t] : kAdvanceInf;
  }
  if (gt == 0) {
    A.n_horizon[b] = hz;
    A.n_pdiag[b] = row >= 0 ? A.h_scal[(size_t)row * 3] : 0.0;
    if (A.n_lf) A.n_lf[b] = row >= 0 ? A.h_scal[(size_t)row * 3 + 1] : 0.0;
    if (A.n_dc) A.n_dc[b] = row >= 0 ? A.h_scal[(size_t)row * 3 + 2] : 0.0;
    if (A.n_dfloor) {
      double sum = 0.0;   // increasing i, one rounding per addition
      for (int i = 0; i < N; ++i) sum = sum + ap[i];
      const double kw = A.kw_per_amp * sum;
      const double old = A.dfloor ? A.dfloor[b] : 0.0;
      A.n_dfloor[b] = kw > old ? kw : old;
    }
    A.flags[b] = flag;
  }
}

hipError_t launch_advance(const AdvanceArgs& a, hipStream_t st);   // the CLOCK variant iff a.c_series is given

}  // namespace acnqp
