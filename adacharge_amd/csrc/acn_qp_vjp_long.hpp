// Gradients through the solve at horizons 33 ... 288 on sites of up to 64 EVSEs (acnqp_vjp_device / acnqp_vjp_host behind
// acnqp_set_long_vjp, include/acn_qp.h): the adjoint of acn_qp_vjp.hpp -- ONE Newton round of the polish
// with g = dL/dx in place of pd x + q and zero constraint residuals -- with the storage of polish_long_kernel
// (acn_qp_polish_long.hpp).  Thread (i = tid / 4, h = tid % 4) LOOPS over its strip of EVSE i's periods; the state lives in
// the workgroup's slab of global memory and in LDS, both carved by PolishLongLayout (acn_qp_polslab.hpp): the row tables,
// the packed per-period blocks, the status bytes, CS and the tight rows' bytes in the slab; G, each wave's block in work,
// Z_t, the capacitance matrix (where it fits), the session tables and the reductions in LDS.  The tables hold the worst
// case of the shape, so verdict 2 (rows) cannot occur.  Every step on the tables is a call into acn_qp_polish_steps.hpp;
// steps 6a ... 6e, which the long polish writes out between its phase clocks, are restated below for a kernel that has none
// (pol_step6_slab), as pol_step6_lds restates the short polish's for vjp_kernel.
//
// A backward is a whole batch: workgroup w takes the problems w, w + grid, ... in turn -- no queue, no atomics -- and reuses
// its slab from one to the next.  Nothing of a previous problem is read: every table a problem reads, it first writes
// (the (N, Tm) arrays and bytes by the strips, which cover every period; U, NU and the tight rows over all of (rows, Tm);
// the row tables up to the rows counted, the blocks up to the doubles counted, the capacitance matrix up to its columns;
// COLOF at every (EVSE, slot) that CS names).
//
// Determinism: every sum runs in a fixed order (a thread's strip in period order, a quad's two exchanges, a table row's
// loop, a period's columns in EVSE order); workgroups share nothing and no floating-point atomic is used: the same problem
// gives the same bits in any batch, at any position and under any grid.  tests/vjp_spec.py restates the system densely.
#pragma once
#include "acn_qp_polslab.hpp"
#include "acn_qp_vjp.hpp"

namespace acnqp {

constexpr long long kVjpLongScratchBytes = 512ll << 20;   // slabs of one launch at most (the worst shape, 64 x 288 x 4 with
                                                          // 48 rows, takes 5.0 MiB per workgroup: 102 workgroups)

struct VjpLongArgs {
  VjpArgs v;      // as for vjp_kernel; max_rows, max_sess, blk_doubles: the worst case of the shape (PolishLongLayout)
  double* slab;   // gridDim.x slabs of PolishLongLayout::slab_total doubles
};

// the tables of a long-horizon launch, handed to pol_step6_slab
struct VjpLongTables {
  const double* Gs;
  const signed char* CS;
  const int *TSTART, *BOFF, *SI, *SKS, *S0, *S1, *COLOF;
  int *ACT, *ACTI, *MISC;
  double *BLK, *CAP, *ZB, *ZV, *DI;
  const double* SISQ;
  double *WB, *WV, *WD;   // this wave's block in work, its right-hand side, 1 / D
  double *TB, *TD;        // wave 0's block in work and 1 / D: the period's block of 6c
};

// (6a) ... (6e) with the blocks in the slab, phase for phase as polish_long_kernel stages them: a wave per block, factored and
// solved while it sits in the wave's LDS; the capacitance matrix accumulated from the columns that touch a period, in
// EVSE order; C w = V' y; lam = y + B^-1 V w.  In: LAM = rhs, BLK / CAP as pol_step5 left them, MISC[3] = 0.  Out: LAM = lam,
// RDG = 1 / D of the blocks; RCA is scratch.  False: a pivot is not positive (block-uniform).  Ends behind a barrier.
__device__ __forceinline__ bool pol_step6_slab(const PolRows& R, const VjpLongTables& W, int N, int Tm, int M, int m, int nsa, int tid) {
  const int wave_ = tid >> 6, lane_ = tid & 63;
  // (6a, 6b)
  for (int t = wave_; t < Tm; t += 4) {
    const int mt = W.TSTART[t + 1] - W.TSTART[t], a0 = W.TSTART[t];
    if (mt == 0) continue;   // (wave-uniform)
    double* gblk = W.BLK + W.BOFF[t];
    for (int p = lane_; p < mt * (mt + 1) / 2; p += 64) W.WB[p] = gblk[p];
    for (int k = lane_; k < mt; k += 64) W.WV[k] = R.LAM[a0 + k];
    pol_wave_sync();
    if (!pol_block_factor(W.WB, mt, lane_)) { if (lane_ == 0) W.MISC[3] = 1; pol_wave_sync(); continue; }
    for (int k = lane_; k < mt; k += 64) W.WD[k] = 1.0 / W.WB[k * (k + 1) / 2 + k];
    pol_wave_sync();
    pol_block_solve(W.WB, W.WD, W.WV, mt, lane_);
    for (int p = lane_; p < mt * (mt + 1) / 2; p += 64) gblk[p] = W.WB[p];
    for (int k = lane_; k < mt; k += 64) { R.RDG[a0 + k] = W.WD[k]; R.LAM[a0 + k] = W.WV[k]; }
    pol_wave_sync();   // (the wave's next block reuses WB / WV / WD)
  }
  __syncthreads();
  if (W.MISC[3]) return false;
  // (6c)
  for (int c = tid; c < nsa; c += kPolThreads) {
    const int ic = W.SI[c], ks = W.SKS[c];
    double z = 0;
    for (int t = W.S0[c]; t < W.S1[c]; ++t)
      if (W.CS[(size_t)ic * Tm + t] == ks)
        for (int a = W.TSTART[t]; a < W.TSTART[t + 1]; ++a) z += R.at(W.Gs, N, M, a, ic) * R.LAM[a];
    W.ZV[c] = z * W.SISQ[c];
  }
  if (nsa > 0) {   // (block-uniform)
    for (int t = 0; t < Tm; ++t) {
      const int mt = W.TSTART[t + 1] - W.TSTART[t], a0 = W.TSTART[t];
      if (mt == 0) continue;   // (block-uniform)
      if (wave_ == 0) {
        const int cs = lane_ < N ? (int)W.CS[(size_t)lane_ * Tm + t] : -2;
        const bool on = cs >= 0;
        const unsigned long long bal = __ballot(on);
        if (on) {
          const int p = __popcll(bal & ((1ull << lane_) - 1ull));
          W.ACT[p] = W.COLOF[lane_ * 4 + cs]; W.ACTI[p] = lane_;
        }
        if (lane_ == 0) W.MISC[4] = __popcll(bal);
      }
      const double* gblk = W.BLK + W.BOFF[t];
      for (int p = tid; p < mt * (mt + 1) / 2; p += kPolThreads) W.TB[p] = gblk[p];
      for (int k = tid; k < mt; k += kPolThreads) W.TD[k] = R.RDG[a0 + k];
      __syncthreads();
      const int na = W.MISC[4];
      if (na > 0) {   // (block-uniform)
        for (int idx = tid; idx < mt * na; idx += kPolThreads) {
          const int k = idx / na, p = idx - k * na;
          W.ZB[k * kPolLongActive + p] = R.at(W.Gs, N, M, a0 + k, W.ACTI[p]) * W.SISQ[W.ACT[p]];
        }
        __syncthreads();
        if (tid < na) {
          for (int k = 0; k < mt; ++k) {
            const double zk = W.ZB[k * kPolLongActive + tid] * W.TD[k];
            for (int r = k + 1; r < mt; ++r) W.ZB[r * kPolLongActive + tid] -= W.TB[r * (r + 1) / 2 + k] * zk;
          }
        }
        __syncthreads();
        for (int p = tid; p < na * (na + 1) / 2; p += kPolThreads) {
          const int pr = pol_tri_row(p);
          const int pc = p - pr * (pr + 1) / 2;
          double sacc = 0;
          for (int k = 0; k < mt; ++k) sacc += W.ZB[k * kPolLongActive + pr] * W.TD[k] * W.ZB[k * kPolLongActive + pc];
          const int c = W.ACT[pr], c2 = W.ACT[pc];   // (EVSE order is column order: c >= c2)
          W.CAP[c * (c + 1) / 2 + c2] -= sacc;
        }
      }
      __syncthreads();
    }
  }
  // (6d)
  if (!pol_step6d(W.CAP, W.ZV, W.DI, nsa, tid)) return false;
  // (6e)
  for (int a = tid; a < m; a += kPolThreads) {
    const int ta = R.RT[a];
    double sacc = 0;
    for (int e = 0; e < N; ++e) {   // (EVSE order is column order)
      const int cs = W.CS[(size_t)e * Tm + ta];
      if (cs >= 0) { const int c = W.COLOF[e * 4 + cs]; sacc += R.at(W.Gs, N, M, a, e) * W.SISQ[c] * W.ZV[c]; }
    }
    R.RCA[a] = sacc;
  }
  __syncthreads();
  for (int t = wave_; t < Tm; t += 4) {
    const int mt = W.TSTART[t + 1] - W.TSTART[t], a0 = W.TSTART[t];
    if (mt == 0) continue;
    const double* gblk = W.BLK + W.BOFF[t];
    for (int p = lane_; p < mt * (mt + 1) / 2; p += 64) W.WB[p] = gblk[p];
    for (int k = lane_; k < mt; k += 64) { W.WV[k] = R.RCA[a0 + k]; W.WD[k] = R.RDG[a0 + k]; }
    pol_wave_sync();
    pol_block_solve(W.WB, W.WD, W.WV, mt, lane_);
    for (int k = lane_; k < mt; k += 64) R.LAM[a0 + k] += W.WV[k];
    pol_wave_sync();
  }
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(kPolThreads, 1) void vjp_long_kernel(const VjpLongArgs AL) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vjp_long_smem[];
  double* sm = reinterpret_cast<double*>(vjp_long_smem);
  const VjpArgs& A = AL.v;
  const int N = A.N, Tm = A.Tm, K = A.K, M = A.M, Mg = A.Mg;
  const bool soc = A.cone == 1;
  const int nrow = M + (A.has_peak ? 1 : 0);
  const PolishLongLayout L(N, Tm, K, Mg, nrow);
  const int MS = L.max_sess, MR = L.max_rows;
  // ---- the slab of this workgroup (the layout's names; what the adjoint keeps there is said on the right) -----------------
  double* sl = AL.slab + (size_t)blockIdx.x * (size_t)L.slab_total;
  double* X = sl + L.x;     // the point, clamped to its bounds
  double* D = sl + L.d;     // v_free = -P g, then pd x + q + G'y of the point's own stationarity
  double* GV = sl + L.g;    // g on the free variables, zero elsewhere
  double* GX = sl + L.e;    // g on the periods of the horizon, zero beyond
  double* Q = sl + L.q;
  double* RL = sl + L.rn;   // (R' lam)(i, t), on every variable
  double *U = sl + L.u, *NU = sl + L.nu;
  double *RC0 = sl + L.rc0, *RC1 = sl + L.rc1, *RCA = sl + L.rca, *RDG = sl + L.rdg, *LAM = sl + L.lam, *BLK = sl + L.blk;
  int* RJ = reinterpret_cast<int*>(sl + L.itab);
  int* RR = RJ + MR;
  int* RT = RR + MR;
  unsigned char* ST = reinterpret_cast<unsigned char*>(sl + L.btab);   // per (i, t): 1 at lb, 2 at ub, 4 lb == ub
  signed char* CS = reinterpret_cast<signed char*>(ST + (size_t)N * Tm);   // per (i, t): -2 not free, -1 free, k >= 0 free in tight session k
  const PolTightBytes RACT{reinterpret_cast<unsigned char*>(CS + (size_t)N * Tm)};
  const PolRows R{RJ, RR, RT, RC0, RC1, RCA, RDG, LAM};
  // ---- LDS ----------------------------------------------------------------------------------------------------------------
  double *Gs = sm + L.gs, *SISQ = sm + L.sisq, *RED = sm + L.red;
  int* TSTART = reinterpret_cast<int*>(sm + L.ints);
  int* BOFF = TSTART + Tm + 1;
  int* SI = BOFF + Tm + 1;
  int* SKS = SI + MS;
  int* S0 = SKS + MS;
  int* S1 = S0 + MS;
  int* COLOF = S1 + MS;
  int* ACT = COLOF + 4 * N;
  int* ACTI = ACT + kPolLongActive;
  int* MISC = ACTI + kPolLongActive;   // [2] session columns, [3] bad pivot, [4] columns of the period in work

  const int tid = threadIdx.x;
  const int i = tid >> 2, h = tid & 3;
  const int wave_ = tid >> 6;
  const int TQ = (Tm + 3) >> 2;
  const bool iv = i < N;
  const int t0 = iv ? min(h * TQ, Tm) : 0, t1 = iv ? min(h * TQ + TQ, Tm) : 0;   // own strip (a short or empty last one; none without an EVSE)
  const size_t vi = (size_t)(iv ? i : 0) * Tm;
  VjpLongTables W;
  W.Gs = Gs; W.CS = CS; W.TSTART = TSTART; W.BOFF = BOFF; W.SI = SI; W.SKS = SKS; W.S0 = S0; W.S1 = S1; W.COLOF = COLOF;
  W.ACT = ACT; W.ACTI = ACTI; W.MISC = MISC; W.BLK = BLK;
  W.CAP = L.cap_in_lds ? sm + L.lcap : sl + L.cap;
  W.ZB = sm + L.zb; W.ZV = sm + L.zv; W.DI = sm + L.di; W.SISQ = SISQ;
  W.WB = sm + L.wblk + wave_ * L.blk_one;
  W.WV = sm + L.wvec + wave_ * 2 * L.mt_max;
  W.WD = W.WV + L.mt_max;
  W.TB = sm + L.wblk;
  W.TD = sm + L.wvec + L.mt_max;
  for (int k = tid; k < Mg * N; k += kPolThreads) Gs[k] = A.G[k];   // (the site's, once per workgroup)

  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
    __syncthreads();   // (the previous problem's last reads of slab and LDS are over; the first: Gs is written)
    const int st = A.status ? A.status[b] : 1;
    if (st != 1 && st != 5) { vjp_give_up(A, b, nrow, kVjpStatus, tid); continue; }   // neither SOLVED nor SOLVED_INACCURATE (block-uniform)
    const PolSite S{N, Tm, M, Mg, nrow, b, soc, A.limits, A.peak};
    const bool eq = A.s_eq[b] != 0;
    const int T = A.horizon[b];
    const size_t bn = (size_t)b * N * Tm;

    // ---- own variables: the polish's first working set at x; g = dL/dx on the periods of the horizon -----------------------
    double qmax = 0, umax = 0, gmax = 0;
    for (int t = t0; t < t1; ++t) {
      const size_t idx = bn + vi + t;
      const double lo = A.lb[idx], up = fmax(A.ub[idx], lo), qq = A.q[idx];
      const double xx = fmin(fmax(A.x[idx], lo), up);
      const double gg = t < T ? A.gx[idx] : 0.0;
      Q[vi + t] = qq; X[vi + t] = xx; GX[vi + t] = gg;   // (the bounds live on in the status byte alone)
      qmax = fmax(qmax, fabs(qq));
      umax = fmax(umax, up);
      gmax = fmax(gmax, fabs(gg));
      const bool lob = xx <= lo + kPolTolBound;
      const bool hib = xx >= up - kPolTolBound && !lob;
      ST[vi + t] = (unsigned char)((lob ? 1 : 0) | (hib ? 2 : 0) | (up - lo <= kPolTolBound ? 4 : 0));
    }
    const double qraw = pol_block_max(qmax, RED);
    const double ubmax = pol_block_max(umax, RED);
    const double gnorm = fmax(1.0, pol_block_max(gmax, RED));
    const double qn = fmax(1.0, qraw);
    const double pd = effective_pdiag<double>(A.pdiag[b], A.reg_rel, qraw, ubmax, T, false);
    // ---- own sessions (the same on the four threads of the quad): window [soff, send) ----------------------------------------
    int soff[kMaxK], send[kMaxK];
    double smu[kMaxK], nfree[kMaxK];
    bool son[kMaxK];   // the energy row is tight and has free variables: a row of C
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      soff[ks] = 0; send[ks] = 0; smu[ks] = 0;
      double scap = 0;
      bool has = false;
      if (ks < K && iv) {
        const size_t sidx = ((size_t)b * K + ks) * N + i;
        const int off = A.s_off[sidx], len = A.s_len[sidx];
        scap = A.s_cap[sidx];
        has = len > 0;
        soff[ks] = max(off, 0);
        send[ks] = len > 0 ? min(off + len, Tm) : soff[ks];
      }
      double s = 0, nf = 0;
      for (int t = max(t0, soff[ks]); t < min(t1, send[ks]); ++t) {
        s += X[vi + t];
        nf += (ST[vi + t] & 3) == 0 ? 1.0 : 0.0;
      }
      s = pol_quad_sum(s);
      nfree[ks] = pol_quad_sum(nf);
      const bool act = has && (eq || s >= scap - kPolTolBound * fmax(1.0, fabs(scap)));
      son[ks] = act && nfree[ks] > 0;
    }
    // ---- the tight site rows by their multipliers in y ---------------------------------------------------------------------------
    pol_first_guess(S, RACT, A.y, NU, qn, tid);
    // ---- (1) which session a free variable belongs to ------------------------------------------------------------------------------
    for (int t = t0; t < t1; ++t) {
      int c = (ST[vi + t] & 3) == 0 ? -1 : -2;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) c = (c == -1 && son[ks] && t >= soff[ks] && t < send[ks]) ? ks : c;
      CS[vi + t] = (signed char)c;
    }
    __syncthreads();
    // ---- (2) G x -----------------------------------------------------------------------------------------------------------------------
    pol_g_times<size_t>(Gs, X, U, N, Tm, Mg, tid);
    __syncthreads();
    // ---- (3) rows and session columns of the Schur system ---------------------------------------------------------------------------
    pol_step3_rows(S, RACT, R, U, NU, TSTART, MR, qn, pd, RED, tid);
    pol_step3_columns(son, nfree, h == 0 && iv, i, MS, SI, SKS, SISQ, MISC + 2, RED, [&](int c, int ks) {
      S0[c] = soff[ks]; S1[c] = send[ks];   // the column's window, and the column of (EVSE, slot)
      COLOF[i * 4 + ks] = c;
    });
    // ---- (4) v_free = -P g: the caller's g in place of pd x + q, c_E = 0 ---------------------------------------------------------------
    double Eg[kMaxK];
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] = 0;
    for (int t = t0; t < t1; ++t) {
      const bool fr = (ST[vi + t] & 3) == 0;
      const double g = fr ? GX[vi + t] : 0.0;
      GV[vi + t] = g;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] += (fr && t >= soff[ks] && t < send[ks]) ? g : 0.0;
    }
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] = pol_quad_sum(Eg[ks]);
    for (int t = t0; t < t1; ++t) {
      const bool fr = (ST[vi + t] & 3) == 0;
      double pg = GV[vi + t];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) pg -= (son[ks] && fr && t >= soff[ks] && t < send[ks]) ? Eg[ks] / nfree[ks] : 0.0;
      D[vi + t] = -pg;
    }
    __syncthreads();
    const int m = TSTART[Tm], nsa = MISC[2];
    if (m > MR || nsa > MS) { vjp_give_up(A, b, nrow, kVjpRows, tid); continue; }   // (block-uniform; never expected: the tables hold the worst case)
    for (int a = tid; a < m; a += kPolThreads) RCA[a] = 0.0;   // c_A = 0
    if (tid == 0) { pol_block_offsets(TSTART, BOFF, Tm); MISC[3] = 0; }
    __syncthreads();
    const int E = BOFF[Tm];
    if (E > A.blk_doubles) { vjp_give_up(A, b, nrow, kVjpRows, tid); continue; }      // (as above)
    // ---- (5), (6) the Schur system, with the polish's dual regularisation ------------------------------------------------------------
    pol_step5<size_t>(R, Gs, D, CS, TSTART, BOFF, BLK, W.CAP, N, Tm, M, m, E, nsa, pd, RED, tid);
    if (!pol_step6_slab(R, W, N, Tm, M, m, nsa, tid)) { vjp_give_up(A, b, nrow, kVjpPivot, tid); continue; }
    // ---- (7) the step dx = -a and the multipliers -m ---------------------------------------------------------------------------------
    double Ev[kMaxK];
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) Ev[ks] = 0;
    for (int t = t0; t < t1; ++t) {
      double rl = 0;   // at a fixed variable: the column's image under the site rows and the curvature
      for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) {
        const int ja = RJ[a];
        const double c1 = RC1[a];
        const double ra = RC0[a] * Gs[ja * N + i] + (c1 != 0.0 ? c1 * Gs[(ja + M) * N + i] : 0.0);
        rl += LAM[a] * ra;
      }
      RL[vi + t] = rl;
      const bool fr = (ST[vi + t] & 3) == 0;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) Ev[ks] += (fr && t >= soff[ks] && t < send[ks]) ? GV[vi + t] + rl : 0.0;
    }
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      Ev[ks] = pol_quad_sum(Ev[ks]);
      smu[ks] = son[ks] ? -Ev[ks] / nfree[ks] : 0.0;
    }
    // the gradients of q and of the bounds, as they come: dx on the free variables, g - (H a + C'm) at a fixed one
    double r0l = 0;   // |H a + C'm - g| on the free variables, with the multipliers as solved
    for (int t = t0; t < t1; ++t) {
      const int sb = ST[vi + t];
      const bool fr = (sb & 3) == 0, live = t < T;
      const double gl = GV[vi + t] + RL[vi + t];
      double pv = gl, ms = 0;
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        const bool in = t >= soff[ks] && t < send[ks];
        pv -= (son[ks] && fr && in) ? Ev[ks] / nfree[ks] : 0.0;
        ms += in ? smu[ks] : 0.0;
      }
      const double dv = fr ? -pv / pd : 0.0;
      r0l = fmax(r0l, fr ? fabs(pd * dv + gl + ms) : 0.0);
      const double image = GX[vi + t] + RL[vi + t] + ms;
      const size_t idx = bn + vi + t;
      A.gq[idx] = live && fr ? dv : 0.0;
      if (A.glb) A.glb[idx] = live && (sb & 1) ? image : 0.0;
      if (A.gub) A.gub[idx] = live && (sb & 2) ? image : 0.0;
    }
    // ---- the primal point's own multipliers: mu and z from stationarity, for the weak members and the second residual -----------------
    double r1l = 0, nweak = 0, nfr = 0;
    {
      double mp[kMaxK];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) mp[ks] = 0;
      for (int t = t0; t < t1; ++t) {
        double acc = 0;
        for (int j = 0; j < Mg; ++j) acc += Gs[j * N + i] * A.y[((size_t)b * Mg + j) * Tm + t];
        const double rp = pd * X[vi + t] + Q[vi + t] + acc;
        D[vi + t] = rp;   // (own strip; step 5 was the last to read v_free)
        const bool fr = (ST[vi + t] & 3) == 0;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) mp[ks] += (fr && t >= soff[ks] && t < send[ks]) ? rp : 0.0;
      }
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        const double s = pol_quad_sum(mp[ks]);
        mp[ks] = son[ks] ? -s / nfree[ks] : 0.0;
        if (h == 0 && !eq && son[ks] && fabs(mp[ks]) < kPolTolDual * qn) nweak += 1.0;
      }
      for (int t = t0; t < t1; ++t) {
        const int sb = ST[vi + t];
        double z = D[vi + t];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) z += (t >= soff[ks] && t < send[ks]) ? mp[ks] : 0.0;
        if ((sb & 3) == 0) { r1l = fmax(r1l, fabs(z)); nfr += 1.0; }
        else if (!(sb & 4)) nweak += fabs(z) < kPolTolDual * qn ? 1.0 : 0.0;
      }
      // (a tight site row is never weak: it is tight because its multiplier exceeds kPolTolRow qn = kPolTolDual qn)
    }
    const double res0 = pol_block_max(r0l, RED) / gnorm;
    const double res1 = pol_block_max(r1l, RED) / qn;
    const double weak = pol_block_sum(nweak, RED);
    const double nfr_all = pol_block_sum(nfr, RED);
    pol_step9_multipliers(R, NU, m, nrow, Tm, tid);   // NU: the multipliers of the normal rows, zero elsewhere
    __syncthreads();
    // ---- results -------------------------------------------------------------------------------------------------------------------------
    if (h == 0 && iv) {
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks)
        if (ks < K) A.gcap[((size_t)b * K + ks) * N + i] = son[ks] ? -smu[ks] : 0.0;
    }
    for (int k = tid; k < nrow * Tm; k += kPolThreads) A.grow[(size_t)b * nrow * Tm + k] = 0.0 - NU[k];
    if (tid == 0) {
      int32_t* info = A.info + (size_t)b * 4;
      info[0] = kVjpDone; info[1] = m; info[2] = (int)weak; info[3] = (int)nfr_all;
      A.res[(size_t)b * 2] = res0;
      A.res[(size_t)b * 2 + 1] = res1;
    }
  }
}

// (vjp_long_grid and launch_vjp_long, the host's side: declared in acn_qp_vjp.hpp, which every caller includes)

}  // namespace acnqp
