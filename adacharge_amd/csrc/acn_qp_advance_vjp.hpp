// The adjoint of "time passes" (acnqp_advance_vjp_device / _host, include/acn_qp.h): one call of the backward sweep through
// a closed loop solve -> pilots -> advance.  For a scalar L of the applied pilots it takes the state of step s, what
// happened to it, dL/d(applied[s]) and the adjoints of the state of step s + 1, and gives
//   gx          dL/dx of step s's solve (the continuous pilot rule is a clip of x[i][0]): what acnqp_vjp_device takes
//   gcap_carry  the part of dL/d(s_cap of step s) that flows through the next state's caps (cap' = cap - a)
//   garr        dL/d(a_cap) of the arrival records the forward advance admitted
//   gprice      dL/d(series) of the clock cost, accumulated over the calls: q' = q_table + coef * (weight * price)
//
// tests/advance_vjp_spec.py states the rules A1 ... A7 in plain loops; the kernel is held to it BIT FOR BIT (contraction
// is switched off).  Rules 1, 2 and 4 of the forward kernel (acn_qp_advance.hpp) are restated here with the same
// comparisons -- that kernel keeps them inline, and its text is not touched -- and the specification holds both.
//
// One workgroup per problem, sized as the forward kernel's (advance_threads).  A thread owns an EVSE for A3 ... A7: its
// K <= 4 slots live in registers.  A2 is a sum over the EVSEs in increasing i for every period: the lanes are the periods,
// so its order does not depend on the block size.  No atomics: one workgroup owns row b of gprice and the records of its
// own segment, and the calls of a sweep are ordered on the stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "acn_qp_advance.hpp"

namespace acnqp {

constexpr int kAdvVjpMaxK = 4;   // session slots per EVSE (what the vjp kernels serve)

struct AdvanceVjpArgs {
  int B, N, Tm, K;
  // the state of step s and what happened to it
  const int32_t *s_off, *s_len;   // [B][K][N]
  const double* s_cap;            // [B][K][N]
  const double* applied;          // [B][N]; not read at step -1
  const int32_t* status;          // [B] or nullptr; not read at step -1
  const double* x;                // [B][N][Tm]; not read at step -1
  const double* max_pilot;        // [N]; not read at step -1
  const double* gdir;             // [B][N] dL/d applied[s]; not read at step -1
  // the plan
  int step, A, R;
  double done_tol;
  const int32_t* a_seg;           // [B + 1] or nullptr: no arrival in this step
  const int32_t *a_evse, *a_slot, *a_len, *a_rate_seg;
  // the clock cost (CLOCK instantiations only)
  int c_P = 0;
  double c_coef = 0.0;
  const double* c_weight = nullptr;   // [N]
  // the adjoints of the state of step s + 1; a nullptr counts as zeros
  const double* gq_next;          // [B][N][Tm]
  const double *gcap_vjp_next, *gcap_carry_next;   // [B][K][N]
  const int32_t *horizon_next, *flags_next;        // [B]
  // out
  double* gx;                     // [B][N][Tm]; not written at step -1
  double* gcap_carry;             // [B][K][N]
  double* garr;                   // [A]: the records of the problem's segment are written
  double* gprice;                 // [B][c_P], accumulated
};

inline size_t advance_vjp_lds(int N) { return ((size_t)N * 8 + 15) & ~(size_t)15; }

template <int THREADS, bool CLOCK = false>
__global__ __launch_bounds__(THREADS) void advance_vjp_kernel(const AdvanceVjpArgs A) {
#pragma clang fp contract(off)   // every operation of this kernel is rounded once (tests/advance_vjp_spec.py)
  extern __shared__ __attribute__((aligned(16))) char advance_vjp_lds_raw[];
  double* g0 = reinterpret_cast<double*>(advance_vjp_lds_raw);   // [N] gx[i][0]
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int N = A.N, Tm = A.Tm, K = A.K;
  const int n = N * Tm;
  const size_t pb = (size_t)b * n, sb = (size_t)b * K * N;
  const bool first = A.step < 0;   // the advance that builds the first period's problems: nothing was applied

  // ---- A2: the prices the next state's q' read, one period per lane, the EVSEs in increasing i ---------------------------
  if constexpr (CLOCK) {
    const bool row = !(A.flags_next && (A.flags_next[b] & kAdvanceNoRow));
    if (row) {
      int hz = A.horizon_next[b];
      hz = hz < 0 ? 0 : (hz > Tm ? Tm : hz);   // (step + 1 + t < step + 1 + Tm <= c_P: the entry's series_len check)
      const double* gq = A.gq_next + pb;
      double* gp = A.gprice + (size_t)b * A.c_P + (A.step + 1);
      for (int t = gt; t < hz; t += THREADS) {
        double acc = 0.0;
        for (int i = 0; i < N; ++i) acc = acc + A.c_weight[i] * gq[(size_t)i * Tm + t];
        gp[t] = gp[t] + A.c_coef * acc;
      }
    }
  }

  // ---- A1, A3 ... A7: one thread per EVSE ----------------------------------------------------------------------------------
  const int st = (!first && A.status) ? A.status[b] : kAdvSolved;
  const bool served = st == kAdvSolved || st == kAdvSolvedInaccurate;   // rule 1
  int a0 = A.a_seg ? A.a_seg[b] : 0, a1 = A.a_seg ? A.a_seg[b + 1] : 0;
  a0 = a0 < 0 ? 0 : a0;
  a1 = a1 > A.A ? A.A : a1;
  for (int i = gt; i < N; i += THREADS) {
    const double a = (!first && served) ? A.applied[(size_t)b * N + i] : 0.0;
    double G[kAdvVjpMaxK];
    int noff[kAdvVjpMaxK], nlen[kAdvVjpMaxK];
    double ga = first ? 0.0 : A.gdir[(size_t)b * N + i];
#pragma unroll
    for (int k = 0; k < kAdvVjpMaxK; ++k) {
      G[k] = 0.0; noff[k] = 0; nlen[k] = 0;
      if (k < K) {
        const size_t s = sb + (size_t)k * N + i;
        G[k] = (A.gcap_vjp_next ? A.gcap_vjp_next[s] : 0.0) + (A.gcap_carry_next ? A.gcap_carry_next[s] : 0.0);   // A1
        int off = A.s_off[s], len = A.s_len[s];
        double cap = A.s_cap[s];
        bool kept = false, fed = false;
        if (len > 0 && !(off < 0 || off >= Tm || len > Tm - off)) {   // rule 2, as the forward kernel takes it
          if (off > 0) {
            off -= 1;
          } else {
            len -= 1;
            cap = cap - a;
            if (cap < 0.0) cap = 0.0;
            fed = true;
          }
          kept = !(len == 0 || cap <= A.done_tol);
        }
        if (kept) { noff[k] = off; nlen[k] = len; }
        A.gcap_carry[s] = kept ? G[k] : 0.0;          // A4
        if (kept && fed && served) ga = ga - G[k];    // A5
      }
    }
    if (!first) {   // A6: the branches of the continuous pilot rule, max(min(x, max_pilot), 0)
      const double x0 = A.x[pb + (size_t)i * Tm];
      g0[i] = (served && x0 >= 0.0 && x0 <= A.max_pilot[i]) ? ga : 0.0;
    }
    for (int r = a0; r < a1; ++r) {   // A7: rule 4 in record order, serially per EVSE
      const int e = A.a_evse[r];
      if (e != i) {
        if (i == 0 && (e < 0 || e >= N)) A.garr[r] = 0.0;   // (no EVSE owns it: written once, by the thread of EVSE 0)
        continue;
      }
      const int k = A.a_slot[r], len = A.a_len[r];
      const int r0 = A.a_rate_seg[r];
      bool ok = k >= 0 && k < K && len >= 1 && len <= Tm && r0 >= 0 && r0 <= A.R - len;
      double g = 0.0;
#pragma unroll
      for (int kk = 0; kk < kAdvVjpMaxK; ++kk) {
        if (kk < K) {
          if (kk == k && nlen[kk] != 0) ok = false;             // its slot is live
          if (nlen[kk] > 0 && noff[kk] < len) ok = false;       // [0, len) meets a live window of the EVSE
        }
      }
      if (ok) {
#pragma unroll
        for (int kk = 0; kk < kAdvVjpMaxK; ++kk)
          if (kk == k) { noff[kk] = 0; nlen[kk] = len; g = G[kk]; }
      }
      A.garr[r] = g;
    }
  }
  if (first) return;   // (uniform over the workgroup)
  __syncthreads();
  double* gx = A.gx + pb;
  for (int k = gt; k < n; k += THREADS) gx[k] = (k % Tm) == 0 ? g0[k / Tm] : 0.0;
}

hipError_t launch_advance_vjp(const AdvanceVjpArgs& a, hipStream_t st);   // the CLOCK variant iff a.gprice and a.gq_next are given

}  // namespace acnqp
