// Device-side polish: the active-set Newton method that takes over from the ADMM when a problem of a small site
// (N <= 64, horizon <= 32: the shapes of BASELINE.json configs[1]-[3]) has not converged after options.polish_iters
// iterations.  The reference's solver is an interior-point method (ECOS through cvxpy, aco.py:318): 15-25 iterations on
// every instance, no plateau.  A first-order method has one -- the tangentially degenerate congested instances of
// DESIGN.md section 2 turn the ADMM sub-linear -- and until round 4 the answer was two cold 8,000-iteration restarts
// (configs[3] site 3: a launch as long as its slowest problem, 9,800 iterations).  The ADMM iterate is good enough to
// GUESS the optimal working set, though; from there Newton on the KKT conditions converges in a few dozen small dense
// solves whatever the conditioning of the fixed-point map.
//
// Restated line by line in numpy, with the derivation, in oracle/polish_ref.py (the executable specification of this
// kernel); results are checked against the IPM certificates of tests/golden/stalled.npz.
//
// One workgroup of 256 threads per problem.  Thread (i = tid / 4, h = tid % 4) owns the periods [h TQ, (h + 1) TQ) of
// EVSE i, TQ = ceil(Tm / 4) <= 8, in registers: a session's sums are two lane exchanges inside the EVSE's quad.  The site
// rows live in LDS: G, G x, G dx, the rows of the Schur system (normal + tangent row of every tight disc, period-major)
// and its packed lower triangle.
//
// The kernel below reads top to bottom as step 1 ... step 10 of the specification.  What a thread does on its own
// variables and sessions -- register arrays and bit masks, fully unrolled -- is written out here; every step on the LDS
// tables is a call into acn_qp_polish_steps.hpp (PolishArgs and the kPol* constants live there too), with the tight rows
// as PolTightMask and the blocking-constraint codes as PolCode8.  The LDS carve-up, PolishLds, is acn_qp_pollds.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acn_qp_common.hpp"
#include "acn_qp_polclaim.hpp"
#include "acn_qp_polish_steps.hpp"

namespace acnqp {

// kPolTQ: periods per thread, 4 (horizons <= 16) or 8 (<= 32).  Two workgroups per CU: a polish workgroup then takes ONE of
// the two slots the register-resident solver kernel's workgroups take (256 registers, <= 76 KB of LDS on its shapes) and
// starts as soon as any of them ends -- at one per CU (362 registers) it needed a CU to itself and, in the pipelined host
// path, held 32 CUs away from the neighbouring streams' solver launches: -10 % end to end.
template <int kPolTQ>
__global__ __launch_bounds__(kPolThreads, kPolTQ == 4 ? 2 : 1) void polish_kernel(const PolishArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_smem[];
  double* sm = reinterpret_cast<double*>(pol_smem);
  const int N = A.N, Tm = A.Tm, K = A.K, M = A.M, Mg = A.Mg;
  const bool soc = A.cone == 1;
  const int nrow = M + (A.has_peak ? 1 : 0);
  const PolishLds L(N, Tm, Mg, nrow, A.max_rows, A.blk_doubles, A.max_sess);
  const int MS = A.max_sess;
  double *Xs = sm + L.xs, *Ds = sm + L.ds, *Gs = sm + L.gs, *U = sm + L.u, *DU = sm + L.du, *NU = sm + L.nu, *INVN = sm + L.invn;
  double *RC0 = sm + L.rc0, *RC1 = sm + L.rc1, *RCA = sm + L.rca, *RDG = sm + L.rdg, *LAM = sm + L.lam, *RED = sm + L.red;
  double *BLK = sm + L.blk, *CAP = sm + L.cap, *ZB = sm + L.zb, *ZV = sm + L.zv, *SISQ = sm + L.sisq;
  int* RJ = reinterpret_cast<int*>(sm + L.ints);      // ABI row j of the Schur row
  int* RR = RJ + A.max_rows;                           // its site row r (0 .. nrow - 1); tangent rows: -1 - r
  int* RT = RR + A.max_rows;                           // its period
  int* TSTART = RT + A.max_rows;                       // Schur rows of period t: [TSTART[t], TSTART[t + 1])
  int* BOFF = TSTART + Tm + 1;                         // packed block of period t: BLK + BOFF[t]
  const PolTightMask RACT{reinterpret_cast<unsigned*>(BOFF + Tm + 1)};   // per site row: bit t = tight at period t
  int* MISC = reinterpret_cast<int*>(RACT.w + nrow);   // [2] session columns, [3] bad pivot
  int* SI = MISC + 8;                                  // session columns of V: EVSE, slot
  int* SKS = SI + MS;
  signed char* CS = reinterpret_cast<signed char*>(SKS + MS);   // per (i, t): -2 not free, -1 free, k >= 0 free in tight session k
  const PolRows R{RJ, RR, RT, RC0, RC1, RCA, RDG, LAM};
  typedef PolCode8 Code;
  __shared__ int q_slot;

  const int tid = threadIdx.x;
  const int i = tid >> 2, h = tid & 3;
  const int TQ = (Tm + 3) >> 2;
  const bool iv = i < N;

  for (int q_round = 0;; ++q_round) {
    int pos, b;
    if (A.alongside) {   // (block-uniform) thread 0 claims a PUBLISHED entry, or learns that there is nothing more to wait for
      if (tid == 0) q_slot = pol_claim(A.list, A.queue, A.retired, A.expected, A.B, A.max_polls, [] { __builtin_amdgcn_s_sleep(32); });
      __syncthreads();
      pos = __builtin_amdgcn_readfirstlane(q_slot);
      __syncthreads();
      if (pos < 0) break;
      // every thread acquires the entry itself: the solver's x / y / status / iters stores behind it are visible to all of them
      b = __builtin_amdgcn_readfirstlane(__hip_atomic_load(A.list + pos, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT));
      if (b < 0 || b >= A.B) continue;   // (never expected: a claimed entry is a published problem)
    } else {
      pos = pol_next_listed(A, q_round, &q_slot);
      if (pos < 0) break;
      b = A.list[pos];
    }
    if (A.status[b] != kStatusPolish) continue;   // (block-uniform)
    if (tid == 0) atomicAdd(A.stats + 0, 1);
    if (tid == 0 && A.alongside) atomicAdd(A.taken, 1);
    const PolSite S{N, Tm, M, Mg, nrow, b, soc, A.limits, A.peak};
    const bool eq = A.s_eq[b] != 0;
    const double pd_user = A.pdiag[b];

    // ---- own variables ----------------------------------------------------------------------------------------
    double xv[kPolTQ], lbv[kPolTQ], ubv[kPolTQ], qv[kPolTQ], dv[kPolTQ], gv[kPolTQ], ev[kPolTQ];
    unsigned atlb = 0, atub = 0, fixedm = 0, validm = 0;
    double qmax = 0, umax = 0;
#pragma unroll
    for (int k = 0; k < kPolTQ; ++k) {
      const int t = h * TQ + k;
      const bool ok = iv && k < TQ && t < Tm;
      const size_t idx = ((size_t)b * N + (ok ? i : 0)) * Tm + (ok ? t : 0);
      lbv[k] = ok ? A.lb[idx] : 0.0;
      ubv[k] = ok ? fmax(A.ub[idx], lbv[k]) : 0.0;
      qv[k] = ok ? A.q[idx] : 0.0;
      xv[k] = ok ? fmin(fmax(A.x[idx], lbv[k]), ubv[k]) : 0.0;
      dv[k] = 0; gv[k] = 0; ev[k] = 0;
      validm |= ok ? 1u << k : 0u;
      qmax = fmax(qmax, fabs(qv[k]));
      umax = fmax(umax, ubv[k]);
      const bool lo = xv[k] <= lbv[k] + kPolTolBound;
      const bool hi = xv[k] >= ubv[k] - kPolTolBound && !lo;
      atlb |= lo ? 1u << k : 0u;
      atub |= hi ? 1u << k : 0u;
      fixedm |= (ubv[k] - lbv[k] <= kPolTolBound) ? 1u << k : 0u;
    }
    const double qraw = pol_block_max(qmax, RED);
    const double ubmax = pol_block_max(umax, RED);
    const double qn = fmax(1.0, qraw);
    const double pd = effective_pdiag<double>(pd_user, A.reg_rel, qraw, ubmax, A.horizon[b], false);
    // ---- own sessions (the same on the four threads of the quad) ---------------------------------------------------
    unsigned swm[kMaxK];      // bit k: own period k lies in the window
    double scap[kMaxK], smu[kMaxK];
    bool sact[kMaxK], shas[kMaxK];
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      swm[ks] = 0; scap[ks] = 0; smu[ks] = 0; sact[ks] = false; shas[ks] = false;
      if (ks < K && iv) {
        const size_t sidx = ((size_t)b * K + ks) * N + i;
        const int off = A.s_off[sidx], len = A.s_len[sidx];
        scap[ks] = A.s_cap[sidx];
        shas[ks] = len > 0;
#pragma unroll
        for (int k = 0; k < kPolTQ; ++k) {
          const int t = h * TQ + k;
          if (k < TQ && t >= off && t < off + len && t < Tm) swm[ks] |= 1u << k;
        }
      }
      double s = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) s += ((swm[ks] >> k) & 1u) ? xv[k] : 0.0;
      s = pol_quad_sum(s);
      sact[ks] = shas[ks] && (eq || s >= scap[ks] - kPolTolBound * fmax(1.0, fabs(scap[ks])));
    }
    // ---- site data; first guess of the tight site rows from the ADMM's multipliers ----------------------------------
    for (int k = tid; k < Mg * N; k += kPolThreads) Gs[k] = A.G[k];
    pol_first_guess(S, RACT, A.y, NU, qn, tid);
    __syncthreads();

    int why = 4, rounds = 0;   // reason of a failure (index into stats), rounds made
    PolStall stall;
    stall.reset();
    PolClock clk;
    clk.start();
    bool success = false;
    double stat_out = 0, prim_out = 0;
    for (int rnd = 0; rnd < kPolMaxRounds; ++rnd) {
      rounds = rnd + 1;
      const unsigned freem = validm & ~(atlb | atub);
      // ---- (1) x mirror, session projector pieces --------------------------------------------------------------------
      double nfree[kMaxK], cE[kMaxK];
      bool son[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double nf = 0, sx = 0;
#pragma unroll
        for (int k = 0; k < kPolTQ; ++k) {
          const bool inw = (swm[ks] >> k) & 1u;
          nf += (inw && ((freem >> k) & 1u)) ? 1.0 : 0.0;
          sx += inw ? xv[k] : 0.0;
        }
        nfree[ks] = pol_quad_sum(nf);
        cE[ks] = scap[ks] - pol_quad_sum(sx);
        son[ks] = sact[ks] && nfree[ks] > 0;
        if (h == 0 && iv) INVN[i * 4 + ks] = son[ks] ? 1.0 / nfree[ks] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) {
          Xs[i * Tm + t] = xv[k];
          int c = ((freem >> k) & 1u) ? -1 : -2;
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) c = (c == -1 && son[ks] && ((swm[ks] >> k) & 1u)) ? ks : c;
          CS[i * Tm + t] = (signed char)c;
        }
      }
      __syncthreads();
      // ---- (2) G x ------------------------------------------------------------------------------------------------------
      pol_g_times<int>(Gs, Xs, U, N, Tm, Mg, tid);
      __syncthreads();
      // ---- (3) rows of the Schur system, period-major: pair k = t nrow + r of (period, site row) -> 0 / 1 / 2 rows (a tight
      // disc: its normal row and, with a multiplier worth it, its tangent row); offsets by a block-wide exclusive scan
      pol_step3_rows(S, RACT, R, U, NU, TSTART, A.max_rows, qn, pd, RED, tid);
      pol_step3_columns(son, nfree, h == 0 && iv, i, MS, SI, SKS, SISQ, MISC + 2, RED, [](int, int) {});
      // ---- (4) gradient on the free variables, v_free = -P g + pd e ---------------------------------------------------------
      double Eg[kMaxK];
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) gv[k] = ((freem >> k) & 1u) ? pd * xv[k] + qv[k] : 0.0;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < kPolTQ; ++k) s += (((swm[ks] & freem) >> k) & 1u) ? gv[k] : 0.0;
        Eg[ks] = pol_quad_sum(s);
      }
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        double pg = gv[k], e = 0;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          const bool in = son[ks] && (((swm[ks] & freem) >> k) & 1u);
          pg -= in ? Eg[ks] / nfree[ks] : 0.0;
          e += in ? cE[ks] / nfree[ks] : 0.0;
        }
        ev[k] = e;
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) Ds[i * Tm + t] = -pg + pd * e;
      }
      __syncthreads();
      const int m = TSTART[Tm], nsa = MISC[2];
      if (m > A.max_rows || nsa > MS) { why = 2; break; }   // (block-uniform)
      if (tid == 0) { pol_block_offsets(TSTART, BOFF, Tm); MISC[3] = 0; }
      __syncthreads();
      const int E = BOFF[Tm];
      if (E > A.blk_doubles) { why = 2; break; }
      clk.lap(0);
      // ---- (5) rhs = R v_free - pd c_A;  B = R R' + diag + reg I, BLOCK DIAGONAL by period;  C = I ---------------------------
      pol_step5<int>(R, Gs, Ds, CS, TSTART, BOFF, BLK, CAP, N, Tm, M, m, E, nsa, pd, RED, tid);
      clk.lap(1);
      // ---- (6a) L D L' of every block, a wave per block (unit lower L stored unscaled, 1 / D in RDG) ------------------------------
      const int wave_ = tid >> 6, lane_ = tid & 63;
      for (int t = wave_; t < Tm; t += 4) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        double* blk = BLK + BOFF[t];
        if (!pol_block_factor(blk, mt, lane_)) { if (lane_ == 0) MISC[3] = 1; continue; }
        for (int k = lane_; k < mt; k += 64) RDG[a0 + k] = 1.0 / blk[k * (k + 1) / 2 + k];
      }
      __syncthreads();
      if (MISC[3]) { why = 3; break; }
      // ---- (6b) y = B^-1 rhs ---------------------------------------------------------------------------------------------------------
      for (int t = wave_; t < Tm; t += 4) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        if (mt > 0) pol_block_solve(BLK + BOFF[t], RDG + a0, LAM + a0, mt, lane_);
      }
      __syncthreads();
      // ---- (6c) z = V' y;  C = I - V' B^-1 V = I - sum_t Z_t' D_t^-1 Z_t,  Z_t = L_t^-1 V_t, one block at a time ------------------------
      for (int c = tid; c < nsa; c += kPolThreads) {
        const int ic = SI[c], ks = SKS[c];
        double z = 0;
        for (int t = 0; t < Tm; ++t)
          if (CS[ic * Tm + t] == ks)
            for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) z += R.at(Gs, N, M, a, ic) * LAM[a];
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
            const double zk = ZB[k * MS + c] * RDG[a0 + k];
            for (int r = k + 1; r < mt; ++r) ZB[r * MS + c] -= blk[r * (r + 1) / 2 + k] * zk;
          }
        }
        __syncthreads();
        for (int p = tid; p < nsa * (nsa + 1) / 2; p += kPolThreads) {
          const int c = pol_tri_row(p);
          const int c2 = p - c * (c + 1) / 2;
          if (CS[SI[c] * Tm + t] != SKS[c] || CS[SI[c2] * Tm + t] != SKS[c2]) continue;
          double sacc = 0;
          for (int k = 0; k < mt; ++k) sacc += ZB[k * MS + c] * RDG[a0 + k] * ZB[k * MS + c2];
          CAP[p] -= sacc;
        }
        __syncthreads();
      }
      clk.lap(2);
      // ---- (6d) C = L D L' (packed, one barrier per column), C w = V' y ----------------------------------------------------------------
      if (!pol_step6d(CAP, ZV, ZB, nsa, tid)) { why = 3; break; }   // (1 / D of C goes into the Z buffer, free now)
      // ---- (6e) lam = y + B^-1 (V w) ---------------------------------------------------------------------------------------------------
      for (int a = tid; a < m; a += kPolThreads) {
        const int ta = RT[a];
        double sacc = 0;
        for (int c = 0; c < nsa; ++c) {
          const int ic = SI[c];
          if (CS[ic * Tm + ta] == SKS[c]) sacc += R.at(Gs, N, M, a, ic) * SISQ[c] * ZV[c];
        }
        RCA[a] = sacc;
      }
      __syncthreads();
      for (int t = wave_; t < Tm; t += 4) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        if (mt > 0) pol_block_solve(BLK + BOFF[t], RDG + a0, RCA + a0, mt, lane_);
      }
      __syncthreads();
      for (int a = tid; a < m; a += kPolThreads) LAM[a] += RCA[a];
      __syncthreads();
      clk.lap(3);
      // ---- (7) the step ---------------------------------------------------------------------------------------------------------
      double rl[kPolTQ];   // (R' lam)(i, t), and of the NORMAL rows alone (the multipliers' part of the gradient)
      double rn[kPolTQ];
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        rl[k] = 0; rn[k] = 0;
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) {
          for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) {
            const int ja = RJ[a];
            const double c1 = RC1[a];
            const double ra = RC0[a] * Gs[ja * N + i] + (c1 != 0.0 ? c1 * Gs[(ja + M) * N + i] : 0.0);
            rl[k] += LAM[a] * ra;
            rn[k] += RR[a] >= 0 ? LAM[a] * ra : 0.0;
          }
        }
      }
      double Ev[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < kPolTQ; ++k) s += (((swm[ks] & freem) >> k) & 1u) ? gv[k] + rl[k] : 0.0;
        Ev[ks] = pol_quad_sum(s);
        smu[ks] = son[ks] ? -(pd * cE[ks] + Ev[ks]) / nfree[ks] : 0.0;
      }
      double stepl = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        double pv = gv[k] + rl[k];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) pv -= (son[ks] && (((swm[ks] & freem) >> k) & 1u)) ? Ev[ks] / nfree[ks] : 0.0;
        dv[k] = ((freem >> k) & 1u) ? -pv / pd + ev[k] : 0.0;
        stepl = fmax(stepl, fabs(dv[k]));
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) Ds[i * Tm + t] = dv[k];
      }
      __syncthreads();
      pol_g_times<int>(Gs, Ds, DU, N, Tm, Mg, tid);
      __syncthreads();
      clk.lap(4);
      // ---- (8) ratio test against everything outside the working set ---------------------------------------------------------------
      double alpha = 1.0;
      int block = -1;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        if (!((freem >> k) & 1u)) continue;
        const int t = h * TQ + k;
        const double d = dv[k];
        if (d < -1e-14) {
          const double a_ = fmax((lbv[k] - xv[k]) / d, 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolLb, i, t); }
        } else if (d > 1e-14) {
          const double a_ = fmax((ubv[k] - xv[k]) / d, 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolUb, i, t); }
        }
      }
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < kPolTQ; ++k) s += ((swm[ks] >> k) & 1u) ? dv[k] : 0.0;
        const double de = pol_quad_sum(s);
        if (h == 0 && shas[ks] && !sact[ks] && de > 1e-14) {
          const double a_ = fmax(cE[ks] / de, 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolSess, i, ks); }
        }
      }
      pol_step8_rows<PolTightMask, Code>(S, RACT, U, DU, alpha, block, tid);
      pol_block_argmin(alpha, block, RED);
      if (block < 0) alpha = 1.0;
      clk.lap(5);
      // ---- (9) move; the new multipliers; the blocking constraint joins the working set ------------------------------------------------
      double xm = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) { xv[k] += alpha * dv[k]; xm = fmax(xm, fabs(xv[k])); }
      const double step = pol_block_max(stepl, RED);
      const double xmax = pol_block_max(xm, RED);
      pol_step9_multipliers(R, NU, m, nrow, Tm, tid);
      if (block >= 0) {
        const int kind = Code::kind(block), p0 = Code::p0(block), p1 = Code::p1(block);
        if (kind == kPolLb || kind == kPolUb) {
          if (p0 == i && p1 >= h * TQ && p1 < h * TQ + TQ) {
            const int k = p1 - h * TQ;
#pragma unroll
            for (int kk = 0; kk < kPolTQ; ++kk)
              if (kk == k) {
                if (kind == kPolLb) { atlb |= 1u << kk; xv[kk] = lbv[kk]; } else { atub |= 1u << kk; xv[kk] = ubv[kk]; }
              }
          }
        } else if (kind == kPolSess) {
          if (p0 == i) {
#pragma unroll
            for (int ks = 0; ks < kMaxK; ++ks) if (ks == p1) sact[ks] = true;
          }
        } else if (tid == 0) {
          RACT.set(p0, p1, Tm);
        }
      }
      __syncthreads();
      stall.update(block, step);
      const bool conv = stall.converged(block, step, xmax);
      clk.lap(6);
      if (!conv) continue;
      // ---- (10) multipliers of the whole working set: the most negative one leaves; none: verify and finish ---------------------------------
      double worst = -kPolTolDual * qn;
      int who = -1;
      double statl = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        double gr = pd * xv[k] + qv[k] + rn[k];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) gr += ((swm[ks] >> k) & 1u) ? smu[ks] : 0.0;
        gv[k] = gr;
        const int t = h * TQ + k;
        if (!((validm >> k) & 1u)) continue;
        if ((freem >> k) & 1u) { statl = fmax(statl, fabs(gr)); continue; }
        if ((fixedm >> k) & 1u) continue;
        if (((atlb >> k) & 1u) && gr < worst) { worst = gr; who = Code::make(kPolLb, i, t); }
        if (((atub >> k) & 1u) && -gr < worst) { worst = -gr; who = Code::make(kPolUb, i, t); }
      }
      if (!eq && h == 0) {
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks)
          if (sact[ks] && smu[ks] < worst) { worst = smu[ks]; who = Code::make(kPolSess, i, ks); }
      }
      pol_step10_rows<PolTightMask, Code>(RACT, NU, nrow, Tm, worst, who, tid);
      pol_block_argmin(worst, who, RED);
      if (who >= 0) {
        const int kind = Code::kind(who), p0 = Code::p0(who), p1 = Code::p1(who);
        if (kind == kPolLb || kind == kPolUb) {
          if (p0 == i && p1 >= h * TQ && p1 < h * TQ + TQ) {
            const int k = p1 - h * TQ;
            if (kind == kPolLb) atlb &= ~(1u << k); else atub &= ~(1u << k);
          }
        } else if (kind == kPolSess) {
          if (p0 == i) {
#pragma unroll
            for (int ks = 0; ks < kMaxK; ++ks) if (ks == p1) sact[ks] = false;
          }
        } else if (tid == 0) {
          RACT.clear(p0, p1, Tm);
          NU[p0 * Tm + p1] = 0.0;
        }
        stall.reset();
        __syncthreads();
        continue;
      }
      // ---- KKT on the full problem, at the final x: G x again, the discs' normals from it (the step's rows carry the normals of
      // the point BEFORE the step: nu (n_new - n_old) is 4e-8 after a step of 3e-6 A, above the 1e-8 this check asks for)
      double pvl = 0;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < kPolTQ; ++k) s += ((swm[ks] >> k) & 1u) ? xv[k] : 0.0;
        const double d = pol_quad_sum(s) - scap[ks];
        if (shas[ks]) pvl = fmax(pvl, (eq ? fabs(d) : d) / fmax(1.0, fabs(scap[ks])));
      }
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) Xs[i * Tm + t] = xv[k];
      }
      __syncthreads();
      pol_g_times<int>(Gs, Xs, U, N, Tm, Mg, tid);
      __syncthreads();
      pol_kkt_rows(S, U, pvl, tid);
      statl = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        const int t = h * TQ + k;
        if (!((freem >> k) & 1u)) continue;
        double gr = pd * xv[k] + qv[k];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) gr += ((swm[ks] >> k) & 1u) ? smu[ks] : 0.0;
        for (int r = 0; r < nrow; ++r) {
          const double nu = NU[r * Tm + t];
          if (nu == 0.0) continue;
          const int j = S.row_j(r);
          if (S.is_disc(r)) {
            const double u0 = U[j * Tm + t], u1 = U[(j + M) * Tm + t], val = hypot(u0, u1);
            gr += nu * (u0 * Gs[j * N + i] + u1 * Gs[(j + M) * N + i]) / val;
          } else {
            gr += nu * Gs[j * N + i];
          }
        }
        statl = fmax(statl, fabs(gr));
      }
      const double stat = pol_block_max(statl, RED);
      const double pv = pol_block_max(pvl, RED);
      stat_out = stat; prim_out = pv;
      success = stat <= 1e-8 * qn && pv <= 10.0 * kPolTolPrimal;
      why = 5;
      break;
    }
    // ---- results -----------------------------------------------------------------------------------------------------------------------------------
    clk.lap(7);
    if (tid == 0) clk.flush(A.stats, rounds);
    double ol = 0;
    if (success) {
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) {
          A.x[((size_t)b * N + i) * Tm + t] = xv[k];
          ol += (0.5 * pd_user * xv[k] + qv[k]) * xv[k];
        }
      }
    }
    pol_results(A, S, NU, U, success, ol, rounds, why, prim_out, stat_out, RED, tid);
  }
}

}  // namespace acnqp
