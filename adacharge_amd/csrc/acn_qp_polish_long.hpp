// Device-side polish for horizons 33 ... 288 on sites of up to 64 EVSEs: the method of oracle/polish_ref.py (the executable
// specification) with the storage such horizons need.  Every step on the tables -- the rules, tolerances and arithmetic the
// short kernel uses too -- is a call into acn_qp_polish_steps.hpp, with the tight rows as PolTightBytes and the
// blocking-constraint codes as PolCode12; what is written out below is what a thread does on its own strip, and the
// staging of steps 6a ... 6e.
//
// polish_kernel<4 | 8> keeps a thread's periods in registers and a period's flags in 32-bit masks, and everything else in
// LDS.  Here nothing is sized by the horizon in registers and no mask holds periods: thread (i = tid / 4, h = tid % 4) still
// owns the strip [h TQ, (h + 1) TQ) of EVSE i's periods, TQ = ceil(Tm / 4) <= 72, but LOOPS over it with the state in a
// per-workgroup slab of global memory (acn_qp_polslab.hpp: x, dx, g, e, lb, ub, q as (N, Tm); U, DU as (Mg, Tm); NU; the
// status bytes; the row tables; the packed per-period blocks), indexed by workgroup slot like the solver kernels'
// ws_by_slot workspaces and L2-resident for the few problems a launch hands over.  LDS keeps what is reused within a
// round: G, the block in work of each wave, L_t^-1 V_t of the period in work, the capacitance matrix (where it fits),
// the session columns' tables and the reductions.  Every table holds the worst case of the shape, so a problem is never
// given up for `rows`.
//
// What differs from the short kernel beyond storage:
//   - the capacitance matrix is accumulated from the columns that TOUCH a period (at most one per EVSE: the windows of an
//     EVSE's sessions are disjoint), listed per period in EVSE order, not from all pairs of columns;
//   - a block is factored and its first solve is done while it sits in the wave's LDS (same arithmetic, one pass);
//   - a code gives a period 12 bits (ties still go to the smaller code, ordered like (kind, p0, p1)).
#pragma once
#include "acn_qp_polish_steps.hpp"
#include "acn_qp_polslab.hpp"

namespace acnqp {

struct PolishLongArgs {
  PolishArgs p;     // as for polish_kernel (alongside = 0: the long polish runs as a serial launch only); max_rows, max_sess,
                    // blk_doubles: the worst case of the shape (PolishLongLayout)
  double* slab;     // gridDim.x slabs of PolishLongLayout::slab_total doubles
};

__global__ __launch_bounds__(kPolThreads, 1) void polish_long_kernel(const PolishLongArgs AL) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_long_smem[];
  double* sm = reinterpret_cast<double*>(pol_long_smem);
  const PolishArgs& A = AL.p;
  const int N = A.N, Tm = A.Tm, K = A.K, M = A.M, Mg = A.Mg;
  const bool soc = A.cone == 1;
  const int nrow = M + (A.has_peak ? 1 : 0);
  const PolishLongLayout L(N, Tm, K, Mg, nrow);
  const int MS = L.max_sess, MR = L.max_rows;
  // ---- the slab of this workgroup ----------------------------------------------------------------------------------------
  double* sl = AL.slab + (size_t)blockIdx.x * (size_t)L.slab_total;
  double *X = sl + L.x, *D = sl + L.d, *GV = sl + L.g, *EV = sl + L.e, *LB = sl + L.lb, *UB = sl + L.ub, *Q = sl + L.q, *RN = sl + L.rn;
  double *U = sl + L.u, *DU = sl + L.du, *NU = sl + L.nu;
  double *RC0 = sl + L.rc0, *RC1 = sl + L.rc1, *RCA = sl + L.rca, *RDG = sl + L.rdg, *LAM = sl + L.lam, *BLK = sl + L.blk;
  int* RJ = reinterpret_cast<int*>(sl + L.itab);       // ABI row j of the Schur row
  int* RR = RJ + MR;                                   // its site row r (0 .. nrow - 1); tangent rows: -1 - r
  int* RT = RR + MR;                                   // its period
  unsigned char* ST = reinterpret_cast<unsigned char*>(sl + L.btab);   // per (i, t): 1 at lb, 2 at ub, 4 lb == ub
  signed char* CS = reinterpret_cast<signed char*>(ST + (size_t)N * Tm);   // per (i, t): -2 not free, -1 free, k >= 0 free in tight session k
  const PolTightBytes RACT{reinterpret_cast<unsigned char*>(CS + (size_t)N * Tm)};   // per (site row, t): tight
  const PolRows R{RJ, RR, RT, RC0, RC1, RCA, RDG, LAM};
  typedef PolCode12 Code;
  // ---- LDS ----------------------------------------------------------------------------------------------------------------
  double *Gs = sm + L.gs, *ZB = sm + L.zb, *ZV = sm + L.zv, *SISQ = sm + L.sisq, *DI = sm + L.di, *RED = sm + L.red;
  double* CAP = L.cap_in_lds ? sm + L.lcap : sl + L.cap;   // C = I - V' B^-1 V, packed lower
  int* TSTART = reinterpret_cast<int*>(sm + L.ints);   // Schur rows of period t: [TSTART[t], TSTART[t + 1])
  int* BOFF = TSTART + Tm + 1;                         // packed block of period t: BLK + BOFF[t]
  int* SI = BOFF + Tm + 1;                             // session columns of V: EVSE, slot, window [S0, S1)
  int* SKS = SI + MS;
  int* S0 = SKS + MS;
  int* S1 = S0 + MS;
  int* COLOF = S1 + MS;                                // column of (EVSE, slot)
  int* ACT = COLOF + 4 * N;                            // the columns that touch the period in work, in EVSE order; their EVSEs
  int* ACTI = ACT + kPolLongActive;
  int* MISC = ACTI + kPolLongActive;                   // [2] session columns, [3] bad pivot, [4] columns of the period in work
  __shared__ int q_slot;

  const int tid = threadIdx.x;
  const int i = tid >> 2, h = tid & 3;
  const int wave_ = tid >> 6, lane_ = tid & 63;
  const int TQ = (Tm + 3) >> 2;
  const bool iv = i < N;
  const int t0 = iv ? min(h * TQ, Tm) : 0, t1 = iv ? min(h * TQ + TQ, Tm) : 0;   // own strip (a short or empty last one; none without an EVSE)
  const size_t vi = (size_t)(iv ? i : 0) * Tm;
  double* WB = sm + L.wblk + wave_ * L.blk_one;        // the wave's block in work, its right-hand side, 1 / D
  double* WV = sm + L.wvec + wave_ * 2 * L.mt_max;
  double* WD = WV + L.mt_max;

  for (int q_round = 0;; ++q_round) {
    const int pos = pol_next_listed(A, q_round, &q_slot);
    if (pos < 0) break;
    const int b = A.list[pos];
    if (b < 0 || b >= A.B) continue;              // (never expected)
    if (A.status[b] != kStatusPolish) continue;   // (block-uniform)
    if (tid == 0) atomicAdd(A.stats + 0, 1);
    const PolSite S{N, Tm, M, Mg, nrow, b, soc, A.limits, A.peak};
    const bool eq = A.s_eq[b] != 0;
    const double pd_user = A.pdiag[b];

    // ---- own variables -------------------------------------------------------------------------------------------------
    double qmax = 0, umax = 0;
    for (int t = t0; t < t1; ++t) {
      const size_t idx = ((size_t)b * N + i) * Tm + t;
      const double lo = A.lb[idx], up = fmax(A.ub[idx], lo), qq = A.q[idx];
      const double xx = fmin(fmax(A.x[idx], lo), up);
      LB[vi + t] = lo; UB[vi + t] = up; Q[vi + t] = qq; X[vi + t] = xx;
      qmax = fmax(qmax, fabs(qq));
      umax = fmax(umax, up);
      const bool lob = xx <= lo + kPolTolBound;
      const bool hib = xx >= up - kPolTolBound && !lob;
      ST[vi + t] = (unsigned char)((lob ? 1 : 0) | (hib ? 2 : 0) | (up - lo <= kPolTolBound ? 4 : 0));
    }
    const double qraw = pol_block_max(qmax, RED);
    const double ubmax = pol_block_max(umax, RED);
    const double qn = fmax(1.0, qraw);
    const double pd = effective_pdiag<double>(pd_user, A.reg_rel, qraw, ubmax, A.horizon[b], false);
    // ---- own sessions (the same on the four threads of the quad): window [soff, send) ---------------------------------
    int soff[kMaxK], send[kMaxK];
    double scap[kMaxK], smu[kMaxK];
    bool sact[kMaxK], shas[kMaxK];
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      soff[ks] = 0; send[ks] = 0; scap[ks] = 0; smu[ks] = 0; sact[ks] = false; shas[ks] = false;
      if (ks < K && iv) {
        const size_t sidx = ((size_t)b * K + ks) * N + i;
        const int off = A.s_off[sidx], len = A.s_len[sidx];
        scap[ks] = A.s_cap[sidx];
        shas[ks] = len > 0;
        soff[ks] = max(off, 0);
        send[ks] = len > 0 ? min(off + len, Tm) : soff[ks];
      }
      double s = 0;
      for (int t = max(t0, soff[ks]); t < min(t1, send[ks]); ++t) s += X[vi + t];
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
      // ---- (1) session projector pieces; the session column of every free variable ------------------------------------------
      double nfree[kMaxK], cE[kMaxK];
      bool son[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double nf = 0, sx = 0;
        for (int t = max(t0, soff[ks]); t < min(t1, send[ks]); ++t) {
          nf += (ST[vi + t] & 3) == 0 ? 1.0 : 0.0;
          sx += X[vi + t];
        }
        nfree[ks] = pol_quad_sum(nf);
        cE[ks] = scap[ks] - pol_quad_sum(sx);
        son[ks] = sact[ks] && nfree[ks] > 0;
      }
      for (int t = t0; t < t1; ++t) {
        int c = (ST[vi + t] & 3) == 0 ? -1 : -2;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) c = (c == -1 && son[ks] && t >= soff[ks] && t < send[ks]) ? ks : c;
        CS[vi + t] = (signed char)c;
      }
      __syncthreads();
      // ---- (2) G x ------------------------------------------------------------------------------------------------------
      pol_g_times<size_t>(Gs, X, U, N, Tm, Mg, tid);
      __syncthreads();
      // ---- (3) rows of the Schur system, period-major: pair k = t nrow + r of (period, site row) -> 0 / 1 / 2 rows (a tight
      // disc: its normal row and, with a multiplier worth it, its tangent row); offsets by a block-wide exclusive scan
      pol_step3_rows(S, RACT, R, U, NU, TSTART, MR, qn, pd, RED, tid);
      pol_step3_columns(son, nfree, h == 0 && iv, i, MS, SI, SKS, SISQ, MISC + 2, RED, [&](int c, int ks) {
        S0[c] = soff[ks]; S1[c] = send[ks];   // the column's window, and the column of (EVSE, slot)
        COLOF[i * 4 + ks] = c;
      });
      // ---- (4) gradient on the free variables, v_free = -P g + pd e ---------------------------------------------------------
      double Eg[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] = 0;
      for (int t = t0; t < t1; ++t) {
        const bool fr = (ST[vi + t] & 3) == 0;
        const double g = fr ? pd * X[vi + t] + Q[vi + t] : 0.0;
        GV[vi + t] = g;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] += (fr && t >= soff[ks] && t < send[ks]) ? g : 0.0;
      }
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] = pol_quad_sum(Eg[ks]);
      for (int t = t0; t < t1; ++t) {
        const bool fr = (ST[vi + t] & 3) == 0;
        double pg = GV[vi + t], e = 0;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          const bool in = son[ks] && fr && t >= soff[ks] && t < send[ks];
          pg -= in ? Eg[ks] / nfree[ks] : 0.0;
          e += in ? cE[ks] / nfree[ks] : 0.0;
        }
        EV[vi + t] = e;
        D[vi + t] = -pg + pd * e;
      }
      __syncthreads();
      const int m = TSTART[Tm], nsa = MISC[2];
      if (m > MR || nsa > MS) { why = 2; break; }   // (block-uniform; never expected: the tables hold the worst case)
      if (tid == 0) { pol_block_offsets(TSTART, BOFF, Tm); MISC[3] = 0; }
      __syncthreads();
      const int E = BOFF[Tm];
      if (E > A.blk_doubles) { why = 2; break; }    // (as above)
      clk.lap(0);
      // ---- (5) rhs = R v_free - pd c_A;  B = R R' + diag + reg I, BLOCK DIAGONAL by period;  C = I ---------------------------
      pol_step5<size_t>(R, Gs, D, CS, TSTART, BOFF, BLK, CAP, N, Tm, M, m, E, nsa, pd, RED, tid);
      clk.lap(1);
      // ---- (6a, 6b) L D L' of every block and y = B^-1 rhs, a wave per block, the block in the wave's LDS (unit lower L stored
      // unscaled, 1 / D in RDG) ---------------------------------------------------------------------------------------------------
      for (int t = wave_; t < Tm; t += 4) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        if (mt == 0) continue;   // (wave-uniform)
        double* gblk = BLK + BOFF[t];
        for (int p = lane_; p < mt * (mt + 1) / 2; p += 64) WB[p] = gblk[p];
        for (int k = lane_; k < mt; k += 64) WV[k] = LAM[a0 + k];
        pol_wave_sync();
        if (!pol_block_factor(WB, mt, lane_)) { if (lane_ == 0) MISC[3] = 1; pol_wave_sync(); continue; }
        for (int k = lane_; k < mt; k += 64) WD[k] = 1.0 / WB[k * (k + 1) / 2 + k];
        pol_wave_sync();
        pol_block_solve(WB, WD, WV, mt, lane_);
        for (int p = lane_; p < mt * (mt + 1) / 2; p += 64) gblk[p] = WB[p];
        for (int k = lane_; k < mt; k += 64) { RDG[a0 + k] = WD[k]; LAM[a0 + k] = WV[k]; }
        pol_wave_sync();   // (the wave's next block reuses WB / WV / WD)
      }
      __syncthreads();
      if (MISC[3]) { why = 3; break; }
      // ---- (6c) z = V' y;  C = I - V' B^-1 V = I - sum_t Z_t' D_t^-1 Z_t,  Z_t = L_t^-1 V_t, one block at a time, over the
      // columns that touch the period -------------------------------------------------------------------------------------------
      for (int c = tid; c < nsa; c += kPolThreads) {
        const int ic = SI[c], ks = SKS[c];
        double z = 0;
        for (int t = S0[c]; t < S1[c]; ++t)
          if (CS[(size_t)ic * Tm + t] == ks)
            for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) z += R.at(Gs, N, M, a, ic) * LAM[a];
        ZV[c] = z * SISQ[c];
      }
      if (nsa > 0) {   // (block-uniform)
        double* TB = sm + L.wblk;   // the period's block and 1 / D (wave 0's block in work)
        double* TD = sm + L.wvec + L.mt_max;
        for (int t = 0; t < Tm; ++t) {
          const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
          if (mt == 0) continue;   // (block-uniform)
          if (wave_ == 0) {
            const int cs = lane_ < N ? (int)CS[(size_t)lane_ * Tm + t] : -2;
            const bool on = cs >= 0;
            const unsigned long long bal = __ballot(on);
            if (on) {
              const int p = __popcll(bal & ((1ull << lane_) - 1ull));
              ACT[p] = COLOF[lane_ * 4 + cs]; ACTI[p] = lane_;
            }
            if (lane_ == 0) MISC[4] = __popcll(bal);
          }
          const double* gblk = BLK + BOFF[t];
          for (int p = tid; p < mt * (mt + 1) / 2; p += kPolThreads) TB[p] = gblk[p];
          for (int k = tid; k < mt; k += kPolThreads) TD[k] = RDG[a0 + k];
          __syncthreads();
          const int na = MISC[4];
          if (na > 0) {   // (block-uniform)
            for (int idx = tid; idx < mt * na; idx += kPolThreads) {
              const int k = idx / na, p = idx - k * na;
              ZB[k * kPolLongActive + p] = R.at(Gs, N, M, a0 + k, ACTI[p]) * SISQ[ACT[p]];
            }
            __syncthreads();
            if (tid < na) {
              for (int k = 0; k < mt; ++k) {
                const double zk = ZB[k * kPolLongActive + tid] * TD[k];
                for (int r = k + 1; r < mt; ++r) ZB[r * kPolLongActive + tid] -= TB[r * (r + 1) / 2 + k] * zk;
              }
            }
            __syncthreads();
            for (int p = tid; p < na * (na + 1) / 2; p += kPolThreads) {
              const int pr = pol_tri_row(p);
              const int pc = p - pr * (pr + 1) / 2;
              double sacc = 0;
              for (int k = 0; k < mt; ++k) sacc += ZB[k * kPolLongActive + pr] * TD[k] * ZB[k * kPolLongActive + pc];
              const int c = ACT[pr], c2 = ACT[pc];   // (EVSE order is column order: c >= c2)
              CAP[c * (c + 1) / 2 + c2] -= sacc;
            }
          }
          __syncthreads();
        }
      }
      clk.lap(2);
      // ---- (6d) C = L D L' (packed, one barrier per column), C w = V' y ----------------------------------------------------------------
      if (!pol_step6d(CAP, ZV, DI, nsa, tid)) { why = 3; break; }
      // ---- (6e) lam = y + B^-1 (V w) ---------------------------------------------------------------------------------------------------
      for (int a = tid; a < m; a += kPolThreads) {
        const int ta = RT[a];
        double sacc = 0;
        for (int e = 0; e < N; ++e) {   // (EVSE order is column order)
          const int cs = CS[(size_t)e * Tm + ta];
          if (cs >= 0) { const int c = COLOF[e * 4 + cs]; sacc += R.at(Gs, N, M, a, e) * SISQ[c] * ZV[c]; }
        }
        RCA[a] = sacc;
      }
      __syncthreads();
      for (int t = wave_; t < Tm; t += 4) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        if (mt == 0) continue;
        const double* gblk = BLK + BOFF[t];
        for (int p = lane_; p < mt * (mt + 1) / 2; p += 64) WB[p] = gblk[p];
        for (int k = lane_; k < mt; k += 64) { WV[k] = RCA[a0 + k]; WD[k] = RDG[a0 + k]; }
        pol_wave_sync();
        pol_block_solve(WB, WD, WV, mt, lane_);
        for (int k = lane_; k < mt; k += 64) LAM[a0 + k] += WV[k];
        pol_wave_sync();
      }
      __syncthreads();
      clk.lap(3);
      // ---- (7) the step: (R' lam)(i, t), and of the NORMAL rows alone (the multipliers' part of the gradient) ------------------------------
      double Ev[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) Ev[ks] = 0;
      for (int t = t0; t < t1; ++t) {
        double rl = 0, rn = 0;
        for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) {
          const int ja = RJ[a];
          const double c1 = RC1[a];
          const double ra = RC0[a] * Gs[ja * N + i] + (c1 != 0.0 ? c1 * Gs[(ja + M) * N + i] : 0.0);
          rl += LAM[a] * ra;
          rn += RR[a] >= 0 ? LAM[a] * ra : 0.0;
        }
        D[vi + t] = rl;
        RN[vi + t] = rn;
        const bool fr = (ST[vi + t] & 3) == 0;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) Ev[ks] += (fr && t >= soff[ks] && t < send[ks]) ? GV[vi + t] + rl : 0.0;
      }
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        Ev[ks] = pol_quad_sum(Ev[ks]);
        smu[ks] = son[ks] ? -(pd * cE[ks] + Ev[ks]) / nfree[ks] : 0.0;
      }
      double stepl = 0;
      for (int t = t0; t < t1; ++t) {
        const bool fr = (ST[vi + t] & 3) == 0;
        double pv = GV[vi + t] + D[vi + t];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) pv -= (son[ks] && fr && t >= soff[ks] && t < send[ks]) ? Ev[ks] / nfree[ks] : 0.0;
        const double dv = fr ? -pv / pd + EV[vi + t] : 0.0;
        stepl = fmax(stepl, fabs(dv));
        D[vi + t] = dv;
      }
      __syncthreads();
      pol_g_times<size_t>(Gs, D, DU, N, Tm, Mg, tid);
      __syncthreads();
      clk.lap(4);
      // ---- (8) ratio test against everything outside the working set ---------------------------------------------------------------
      double alpha = 1.0;
      int block = -1;
      double de[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) de[ks] = 0;
      for (int t = t0; t < t1; ++t) {
        const double d = D[vi + t];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) de[ks] += (t >= soff[ks] && t < send[ks]) ? d : 0.0;
        if ((ST[vi + t] & 3) != 0) continue;
        if (d < -1e-14) {
          const double a_ = fmax((LB[vi + t] - X[vi + t]) / d, 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolLb, i, t); }
        } else if (d > 1e-14) {
          const double a_ = fmax((UB[vi + t] - X[vi + t]) / d, 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolUb, i, t); }
        }
      }
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        const double des = pol_quad_sum(de[ks]);
        if (h == 0 && shas[ks] && !sact[ks] && des > 1e-14) {
          const double a_ = fmax(cE[ks] / des, 0.0);
          if (a_ < alpha) { alpha = a_; block = Code::make(kPolSess, i, ks); }
        }
      }
      pol_step8_rows<PolTightBytes, Code>(S, RACT, U, DU, alpha, block, tid);
      pol_block_argmin(alpha, block, RED);
      if (block < 0) alpha = 1.0;
      clk.lap(5);
      // ---- (9) move; the new multipliers; the blocking constraint joins the working set ------------------------------------------------
      double xm = 0;
      for (int t = t0; t < t1; ++t) {
        const double xn = X[vi + t] + alpha * D[vi + t];
        X[vi + t] = xn;
        xm = fmax(xm, fabs(xn));
      }
      const double step = pol_block_max(stepl, RED);
      const double xmax = pol_block_max(xm, RED);
      pol_step9_multipliers(R, NU, m, nrow, Tm, tid);
      if (block >= 0) {
        const int kind = Code::kind(block), p0 = Code::p0(block), p1 = Code::p1(block);
        if (kind == kPolLb || kind == kPolUb) {
          if (iv && p0 == i && p1 >= t0 && p1 < t1) {
            if (kind == kPolLb) { ST[vi + p1] |= 1; X[vi + p1] = LB[vi + p1]; } else { ST[vi + p1] |= 2; X[vi + p1] = UB[vi + p1]; }
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
      for (int t = t0; t < t1; ++t) {
        const int st = ST[vi + t];
        if ((st & 3) == 0 || (st & 4)) continue;
        double gr = pd * X[vi + t] + Q[vi + t] + RN[vi + t];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) gr += (t >= soff[ks] && t < send[ks]) ? smu[ks] : 0.0;
        if ((st & 1) && gr < worst) { worst = gr; who = Code::make(kPolLb, i, t); }
        if ((st & 2) && -gr < worst) { worst = -gr; who = Code::make(kPolUb, i, t); }
      }
      if (!eq && h == 0) {
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks)
          if (sact[ks] && smu[ks] < worst) { worst = smu[ks]; who = Code::make(kPolSess, i, ks); }
      }
      pol_step10_rows<PolTightBytes, Code>(RACT, NU, nrow, Tm, worst, who, tid);
      pol_block_argmin(worst, who, RED);
      if (who >= 0) {
        const int kind = Code::kind(who), p0 = Code::p0(who), p1 = Code::p1(who);
        if (kind == kPolLb || kind == kPolUb) {
          if (iv && p0 == i && p1 >= t0 && p1 < t1) ST[vi + p1] &= (unsigned char)(kind == kPolLb ? ~1 : ~2);
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
      // the point BEFORE the step) ------------------------------------------------------------------------------------------------------
      double pvl = 0;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double s = 0;
        for (int t = max(t0, soff[ks]); t < min(t1, send[ks]); ++t) s += X[vi + t];
        const double d = pol_quad_sum(s) - scap[ks];
        if (shas[ks]) pvl = fmax(pvl, (eq ? fabs(d) : d) / fmax(1.0, fabs(scap[ks])));
      }
      __syncthreads();
      pol_g_times<size_t>(Gs, X, U, N, Tm, Mg, tid);
      __syncthreads();
      pol_kkt_rows(S, U, pvl, tid);
      double statl = 0;
      for (int t = t0; t < t1; ++t) {
        if ((ST[vi + t] & 3) != 0) continue;
        double gr = pd * X[vi + t] + Q[vi + t];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) gr += (t >= soff[ks] && t < send[ks]) ? smu[ks] : 0.0;
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
      for (int t = t0; t < t1; ++t) {
        const double xx = X[vi + t];
        A.x[((size_t)b * N + i) * Tm + t] = xx;
        ol += (0.5 * pd_user * xx + Q[vi + t]) * xx;
      }
    }
    pol_results(A, S, NU, U, success, ol, rounds, why, prim_out, stat_out, RED, tid);
  }
}

}  // namespace acnqp
