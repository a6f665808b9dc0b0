// Device-side polish for sites of 65 ... 1,024 EVSEs at horizons <= 48 (the large-site kernel's shapes, acn_qp_stream.hpp):
// the method of oracle/polish_ref.py (the executable specification) with the storage such sites need.  Every step on the
// tables that holds at any N is a call into acn_qp_polish_steps.hpp, exactly as polish_long_kernel calls it (the tight rows
// as PolTightBytes, the blocking-constraint codes as PolCode12: 16 bits for an EVSE); what is written out below is what a
// thread does on its own strip, the staging of steps 6a ... 6e, and the steps that assumed N <= 64.
//
// It runs BEHIND the solver launch, on the problems that launch ended MAX_ITER or SOLVED_INACCURATE, from the x and y the
// solver kernel wrote for its best pass (acn_qp_api.hip: launch_wide_polish; DESIGN.md 2.3 has why so late), as a serial
// launch only: nothing polls, every loop is bounded (96 rounds, counted pivots).
//
// The thread map is the long kernel's inside a loop over EVSE tiles of 64: thread (tid / 4, h = tid % 4) owns the strip
// [h TQ, (h + 1) TQ) of the periods of EVSE i0 + tid / 4, TQ = ceil(Tm / 4) <= 12; what the quad knows of its EVSE's
// sessions is reloaded per tile -- windows and caps from the caller's arrays, the rest from the slab (PolishWideLayout).
// What differs from the long kernel beyond that (acn_qp_polwide.hpp has the storage side of each):
//   - G is read from global memory (no LDS copy); G x and G dx are a wave per output, the lanes striding over the EVSEs;
//   - the columns that touch a period are listed by a block-wide scan over all EVSEs, not by one wave's ballot;
//   - L_t^-1 V_t is staged in the slab, a thread per column;
//   - the capacitance matrix's solves go column by column with every thread updating entries, not a thread per column;
//   - a working-set change is made by thread 0 in the slab's tables (no thread keeps a session's flags in registers);
//   - a polish that gives up leaves the problem as the solver left it, `iters` included: no launch follows that
//     would overwrite it.
#pragma once
#include "acn_qp_polish_steps.hpp"
#include "acn_qp_polwide.hpp"

namespace acnqp {

struct PolishWideArgs {
  PolishArgs p;     // as for polish_kernel (alongside = 0: a serial launch only); max_rows, max_sess, blk_doubles: the worst
                    // case of the shape (PolishWideLayout)
  double* slab;     // gridDim.x slabs of PolishWideLayout::slab_total doubles
};

// ---- the launch path's two small kernels (acn_qp_api.hip) ----------------------------------------------------------------
// The list: the problems the solver launch ended MAX_ITER (2) or SOLVED_INACCURATE (5), in problem order (ONE workgroup: an
// ordered compaction).  Their status is saved and set to kStatusPolish; *count = the list's length.
__global__ __launch_bounds__(kPolThreads) void polish_wide_list_kernel(int32_t* status, int32_t* saved, int32_t* list, int32_t* count, int B) {
  __shared__ double red[4];
  int base = 0;
  for (int b0 = 0; b0 < B; b0 += kPolThreads) {
    const int b = b0 + (int)threadIdx.x;
    const int st = b < B ? status[b] : 0;
    const bool open = st == 2 || st == 5;
    int total;
    const int pos = pol_block_scan(open ? 1 : 0, base, total, red);
    if (open) { saved[b] = st; status[b] = kStatusPolish; list[pos] = b; }
    base += total;
  }
  if (threadIdx.x == 0) *count = base;
}
// ... and back: what the polish did not solve gets the status the solver gave it
__global__ __launch_bounds__(kPolThreads) void polish_wide_restore_kernel(int32_t* status, const int32_t* saved, const int32_t* list,
                                                                          const int32_t* count, int B) {
  const int n = min(*count, B);
  for (int pos = blockIdx.x * kPolThreads + threadIdx.x; pos < n; pos += gridDim.x * kPolThreads) {
    const int b = list[pos];
    if (b >= 0 && b < B && status[b] == kStatusPolish) status[b] = saved[b];
  }
}

// out[j, t] = sum_e G[j, e] v[e, t] with G in global memory: a wave per output, the lanes striding over the EVSEs
__device__ __forceinline__ void polw_g_times(const double* G, const double* v, double* out, int N, int Tm, int Mg, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  for (int k = wave; k < Mg * Tm; k += 4) {
    const int j = k / Tm, t = k - j * Tm;
    double s = 0;
    for (int e = lane; e < N; e += 64) s += G[(size_t)j * N + e] * v[(size_t)e * Tm + t];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[k] = s;
  }
}

// (6d) at any number of columns: C = L D L' (packed, one barrier per column), C w = V' y -- ZV holds V' y on entry and w on
// return; DI: nsa doubles of room for 1 / D.  The solves go column by column and every thread updates entries.  False: a
// pivot is not positive (block-uniform: every thread reads the same entry).
__device__ __forceinline__ bool polw_step6d(double* CAP, double* ZV, double* DI, int nsa, int tid) {
  bool bad_pivot = false;
  for (int k = 0; k < nsa; ++k) {
    __syncthreads();
    const double piv = CAP[(size_t)k * (k + 1) / 2 + k];
    if (!(piv > 0.0)) { bad_pivot = true; break; }
    const double pinv = 1.0 / piv;
    for (int rr = k + 1 + (tid >> 4); rr < nsa; rr += 16) {
      double* row = CAP + (size_t)rr * (rr + 1) / 2;
      const double lr = row[k] * pinv;
      for (int c = k + 1 + (tid & 15); c <= rr; c += 16) row[c] -= lr * CAP[(size_t)c * (c + 1) / 2 + k];
    }
  }
  if (bad_pivot) return false;
  __syncthreads();
  for (int k = tid; k < nsa; k += kPolThreads) DI[k] = 1.0 / CAP[(size_t)k * (k + 1) / 2 + k];
  __syncthreads();
  for (int k = 0; k < nsa; ++k) {          // forward: L z = V' y
    const double zk = ZV[k] * DI[k];
    for (int r = k + 1 + tid; r < nsa; r += kPolThreads) ZV[r] -= CAP[(size_t)r * (r + 1) / 2 + k] * zk;
    __syncthreads();
  }
  for (int r = tid; r < nsa; r += kPolThreads) ZV[r] *= DI[r];
  __syncthreads();
  for (int k = nsa - 1; k > 0; --k) {      // backward: L' w = D^-1 z
    const double xk = ZV[k];
    const double* row = CAP + (size_t)k * (k + 1) / 2;
    for (int c = tid; c < k; c += kPolThreads) ZV[c] -= row[c] * DI[c] * xk;
    __syncthreads();
  }
  return true;
}

// what a quad knows of its EVSE's sessions: windows [soff, send) and caps from the caller's arrays (the same on its four threads)
struct PolwSess {
  int soff[kMaxK], send[kMaxK];
  double scap[kMaxK];
  bool shas[kMaxK];
  __device__ __forceinline__ void load(const PolishArgs& A, int b, int i, bool iv) {
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      soff[ks] = 0; send[ks] = 0; scap[ks] = 0; shas[ks] = false;
      if (ks < A.K && iv) {
        const size_t sidx = ((size_t)b * A.K + ks) * A.N + i;
        const int off = A.s_off[sidx], len = A.s_len[sidx];
        scap[ks] = A.s_cap[sidx];
        shas[ks] = len > 0;
        soff[ks] = max(off, 0);
        send[ks] = len > 0 ? min(off + len, A.Tm) : soff[ks];
      }
    }
  }
};
constexpr unsigned char kPolwTight = 1, kPolwColumn = 2;   // session flags: in the working set; a column of V this round

__global__ __launch_bounds__(kPolThreads, 1) void polish_wide_kernel(const PolishWideArgs AW) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_wide_smem[];
  double* sm = reinterpret_cast<double*>(pol_wide_smem);
  const PolishArgs& A = AW.p;
  const int N = A.N, Tm = A.Tm, K = A.K, M = A.M, Mg = A.Mg;
  const bool soc = A.cone == 1;
  const int nrow = M + (A.has_peak ? 1 : 0);
  const PolishWideLayout L(N, Tm, K, Mg, nrow);
  const int MS = L.max_sess, MR = L.max_rows;
  const double* Gs = A.G;   // (global memory: Mg x N does not fit in LDS)
  // ---- the slab of this workgroup ----------------------------------------------------------------------------------------
  double* sl = AW.slab + (size_t)blockIdx.x * (size_t)L.slab_total;
  double *X = sl + L.x, *D = sl + L.d, *GV = sl + L.g, *EV = sl + L.e, *LB = sl + L.lb, *UB = sl + L.ub, *Q = sl + L.q, *RN = sl + L.rn;
  double *U = sl + L.u, *DU = sl + L.du, *NU = sl + L.nu;
  double *RC0 = sl + L.rc0, *RC1 = sl + L.rc1, *RCA = sl + L.rca, *RDG = sl + L.rdg, *LAM = sl + L.lam, *BLK = sl + L.blk;
  double *ZB = sl + L.zb, *CAP = sl + L.cap, *SNF = sl + L.snf, *SCE = sl + L.sce, *SMU = sl + L.smu;
  int* RJ = reinterpret_cast<int*>(sl + L.itab);       // ABI row j of the Schur row
  int* RR = RJ + MR;                                   // its site row r (0 .. nrow - 1); tangent rows: -1 - r
  int* RT = RR + MR;                                   // its period
  unsigned char* ST = reinterpret_cast<unsigned char*>(sl + L.btab);   // per (i, t): 1 at lb, 2 at ub, 4 lb == ub
  signed char* CS = reinterpret_cast<signed char*>(ST + (size_t)N * Tm);   // per (i, t): -2 not free, -1 free, k >= 0 free in tight session k
  unsigned char* RACTB = reinterpret_cast<unsigned char*>(CS + (size_t)N * Tm);
  const PolTightBytes RACT{RACTB};                     // per (site row, t): tight
  unsigned char* SFL = RACTB + (size_t)nrow * Tm;      // per (i, slot): kPolwTight | kPolwColumn
  const PolRows R{RJ, RR, RT, RC0, RC1, RCA, RDG, LAM};
  typedef PolCode12 Code;
  // ---- LDS ----------------------------------------------------------------------------------------------------------------
  double *ZV = sm + L.zv, *SISQ = sm + L.sisq, *DI = sm + L.di, *RED = sm + L.red;
  int* TSTART = reinterpret_cast<int*>(sm + L.ints);   // Schur rows of period t: [TSTART[t], TSTART[t + 1])
  int* BOFF = TSTART + Tm + 1;                         // packed block of period t: BLK + BOFF[t]
  int* SI = BOFF + Tm + 1;                             // session columns of V: EVSE, slot, window [S0, S1)
  int* SKS = SI + MS;
  int* S0 = SKS + MS;
  int* S1 = S0 + MS;
  int* COLOF = S1 + MS;                                // column of (EVSE, slot)
  int* ACT = COLOF + 4 * N;                            // the columns that touch the period in work, in EVSE order; their EVSEs
  int* ACTI = ACT + N;
  int* MISC = ACTI + N;                                // [3] bad pivot
  __shared__ int q_slot;

  const int tid = threadIdx.x;
  const int h = tid & 3;
  const int wave_ = tid >> 6, lane_ = tid & 63;
  const int TQ = (Tm + 3) >> 2;
  double* WB = sm + L.wblk + wave_ * L.blk_one;        // the wave's block in work, its right-hand side, 1 / D
  double* WV = sm + L.wvec + wave_ * 2 * L.mt_max;
  double* WD = WV + L.mt_max;
  // own strip in the EVSE tile at i0 (a short or empty last strip; none without an EVSE)
#define POLW_TILE(i0)                                                                  \
  const int i = (i0) + (tid >> 2);                                                     \
  const bool iv = i < N;                                                               \
  const int t0 = iv ? min(h * TQ, Tm) : 0, t1 = iv ? min(h * TQ + TQ, Tm) : 0;         \
  const size_t vi = (size_t)(iv ? i : 0) * Tm;                                         \
  const int si = (iv ? i : 0) * 4;                                                     \
  (void)si; (void)vi

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
    for (int i0 = 0; i0 < N; i0 += 64) {
      POLW_TILE(i0);
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
      // ---- own sessions: the first working set ---------------------------------------------------------------------------
      PolwSess W;
      W.load(A, b, i, iv);
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) {
        double s = 0;
        for (int t = max(t0, W.soff[ks]); t < min(t1, W.send[ks]); ++t) s += X[vi + t];
        s = pol_quad_sum(s);
        const bool sact = W.shas[ks] && (eq || s >= W.scap[ks] - kPolTolBound * fmax(1.0, fabs(W.scap[ks])));
        if (iv && h == 0) { SFL[si + ks] = sact ? kPolwTight : 0; SMU[si + ks] = 0.0; }
      }
    }
    const double qraw = pol_block_max(qmax, RED);
    const double ubmax = pol_block_max(umax, RED);
    const double qn = fmax(1.0, qraw);
    const double pd = effective_pdiag<double>(pd_user, A.reg_rel, qraw, ubmax, A.horizon[b], false);
    // ---- first guess of the tight site rows from the ADMM's multipliers ------------------------------------------------
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
      // ---- (1) session projector pieces; the session column of every free variable; (3) the session columns of V, in
      // (EVSE, slot) order: a block-wide scan per tile, carried from tile to tile ---------------------------------------------
      int ncol = 0;
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        PolwSess W;
        W.load(A, b, i, iv);
        bool son[kMaxK];
        double nfree[kMaxK];
        int cnt = 0;
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          double nf = 0, sx = 0;
          for (int t = max(t0, W.soff[ks]); t < min(t1, W.send[ks]); ++t) {
            nf += (ST[vi + t] & 3) == 0 ? 1.0 : 0.0;
            sx += X[vi + t];
          }
          nfree[ks] = pol_quad_sum(nf);
          const double cE = W.scap[ks] - pol_quad_sum(sx);
          const bool sact = iv && (SFL[si + ks] & kPolwTight);
          son[ks] = sact && nfree[ks] > 0;
          cnt += son[ks] && h == 0 ? 1 : 0;
          if (iv && h == 0) { SNF[si + ks] = nfree[ks]; SCE[si + ks] = cE; }
        }
        for (int t = t0; t < t1; ++t) {
          int c = (ST[vi + t] & 3) == 0 ? -1 : -2;
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) c = (c == -1 && son[ks] && t >= W.soff[ks] && t < W.send[ks]) ? ks : c;
          CS[vi + t] = (signed char)c;
        }
        int total;
        int cpos = pol_block_scan(cnt, ncol, total, RED);   // (its barriers stand between this tile's reads of SFL and the writes below)
        ncol += total;
        if (iv && h == 0) {
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) {
            SFL[si + ks] = (unsigned char)((SFL[si + ks] & kPolwTight) | (son[ks] ? kPolwColumn : 0));
            if (son[ks]) {
              if (cpos < MS) {
                SI[cpos] = i; SKS[cpos] = ks; S0[cpos] = W.soff[ks]; S1[cpos] = W.send[ks];
                COLOF[si + ks] = cpos;
                SISQ[cpos] = 1.0 / sqrt(nfree[ks]);
              }
              ++cpos;
            }
          }
        }
      }
      __syncthreads();
      // ---- (2) G x ------------------------------------------------------------------------------------------------------
      polw_g_times(Gs, X, U, N, Tm, Mg, tid);
      __syncthreads();
      // ---- (3) rows of the Schur system, period-major ------------------------------------------------------------------------
      pol_step3_rows(S, RACT, R, U, NU, TSTART, MR, qn, pd, RED, tid);
      // ---- (4) gradient on the free variables, v_free = -P g + pd e ---------------------------------------------------------
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        PolwSess W;
        W.load(A, b, i, iv);
        bool son[kMaxK];
        double Eg[kMaxK], nfree[kMaxK], cE[kMaxK];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          Eg[ks] = 0;
          son[ks] = iv && (SFL[si + ks] & kPolwColumn);
          nfree[ks] = iv ? SNF[si + ks] : 0.0;
          cE[ks] = iv ? SCE[si + ks] : 0.0;
        }
        for (int t = t0; t < t1; ++t) {
          const bool fr = (ST[vi + t] & 3) == 0;
          const double g = fr ? pd * X[vi + t] + Q[vi + t] : 0.0;
          GV[vi + t] = g;
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] += (fr && t >= W.soff[ks] && t < W.send[ks]) ? g : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) Eg[ks] = pol_quad_sum(Eg[ks]);
        for (int t = t0; t < t1; ++t) {
          const bool fr = (ST[vi + t] & 3) == 0;
          double pg = GV[vi + t], e = 0;
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) {
            const bool in = son[ks] && fr && t >= W.soff[ks] && t < W.send[ks];
            pg -= in ? Eg[ks] / nfree[ks] : 0.0;
            e += in ? cE[ks] / nfree[ks] : 0.0;
          }
          EV[vi + t] = e;
          D[vi + t] = -pg + pd * e;
        }
      }
      __syncthreads();
      const int m = TSTART[Tm], nsa = ncol;
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
          int na = 0;              // the columns that touch the period, in EVSE order: a scan over all EVSEs
          for (int e0 = 0; e0 < N; e0 += kPolThreads) {
            const int e = e0 + tid;
            const int cs = e < N ? (int)CS[(size_t)e * Tm + t] : -2;
            int total;
            const int p = pol_block_scan(cs >= 0 ? 1 : 0, na, total, RED);
            if (cs >= 0) { ACT[p] = COLOF[e * 4 + cs]; ACTI[p] = e; }
            na += total;
          }
          const double* gblk = BLK + BOFF[t];
          for (int p = tid; p < mt * (mt + 1) / 2; p += kPolThreads) TB[p] = gblk[p];
          for (int k = tid; k < mt; k += kPolThreads) TD[k] = RDG[a0 + k];
          __syncthreads();
          if (na > 0) {   // (block-uniform)
            for (int p = tid; p < na; p += kPolThreads) {   // a thread per column: Z = L^-1 V, in the slab (row stride N)
              const int e = ACTI[p];
              const double sq = SISQ[ACT[p]];
              for (int k = 0; k < mt; ++k) ZB[(size_t)k * N + p] = R.at(Gs, N, M, a0 + k, e) * sq;
              for (int k = 0; k < mt; ++k) {
                const double zk = ZB[(size_t)k * N + p] * TD[k];
                for (int r = k + 1; r < mt; ++r) ZB[(size_t)r * N + p] -= TB[r * (r + 1) / 2 + k] * zk;
              }
            }
            __syncthreads();
            for (int p = tid; p < na * (na + 1) / 2; p += kPolThreads) {
              const int pr = pol_tri_row(p);
              const int pc = p - pr * (pr + 1) / 2;
              double sacc = 0;
              for (int k = 0; k < mt; ++k) sacc += ZB[(size_t)k * N + pr] * TD[k] * ZB[(size_t)k * N + pc];
              const int c = ACT[pr], c2 = ACT[pc];   // (EVSE order is column order: c >= c2)
              CAP[(size_t)c * (c + 1) / 2 + c2] -= sacc;
            }
          }
          __syncthreads();
        }
      }
      clk.lap(2);
      // ---- (6d) C = L D L' (packed, one barrier per column), C w = V' y ----------------------------------------------------------------
      if (!polw_step6d(CAP, ZV, DI, nsa, tid)) { why = 3; break; }
      __syncthreads();
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
      // ---- (7) the step: (R' lam)(i, t), and of the NORMAL rows alone (the multipliers' part of the gradient); (8) the ratio
      // test of the own variables and sessions ------------------------------------------------------------------------------------
      double stepl = 0;
      double alpha = 1.0;
      int block = -1;
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        PolwSess W;
        W.load(A, b, i, iv);
        bool son[kMaxK], sact[kMaxK];
        double Ev[kMaxK], nfree[kMaxK], cE[kMaxK], de[kMaxK];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          Ev[ks] = 0; de[ks] = 0;
          son[ks] = iv && (SFL[si + ks] & kPolwColumn);
          sact[ks] = iv && (SFL[si + ks] & kPolwTight);
          nfree[ks] = iv ? SNF[si + ks] : 0.0;
          cE[ks] = iv ? SCE[si + ks] : 0.0;
        }
        for (int t = t0; t < t1; ++t) {
          double rl = 0, rn = 0;
          for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) {
            const int ja = RJ[a];
            const double c1 = RC1[a];
            const double ra = RC0[a] * Gs[(size_t)ja * N + i] + (c1 != 0.0 ? c1 * Gs[(size_t)(ja + M) * N + i] : 0.0);
            rl += LAM[a] * ra;
            rn += RR[a] >= 0 ? LAM[a] * ra : 0.0;
          }
          D[vi + t] = rl;
          RN[vi + t] = rn;
          const bool fr = (ST[vi + t] & 3) == 0;
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) Ev[ks] += (fr && t >= W.soff[ks] && t < W.send[ks]) ? GV[vi + t] + rl : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          Ev[ks] = pol_quad_sum(Ev[ks]);
          if (iv && h == 0) SMU[si + ks] = son[ks] ? -(pd * cE[ks] + Ev[ks]) / nfree[ks] : 0.0;
        }
        for (int t = t0; t < t1; ++t) {
          const bool fr = (ST[vi + t] & 3) == 0;
          double pv = GV[vi + t] + D[vi + t];
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) pv -= (son[ks] && fr && t >= W.soff[ks] && t < W.send[ks]) ? Ev[ks] / nfree[ks] : 0.0;
          const double dv = fr ? -pv / pd + EV[vi + t] : 0.0;
          stepl = fmax(stepl, fabs(dv));
          D[vi + t] = dv;
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) de[ks] += (t >= W.soff[ks] && t < W.send[ks]) ? dv : 0.0;
          if (!fr) continue;
          if (dv < -1e-14) {
            const double a_ = fmax((LB[vi + t] - X[vi + t]) / dv, 0.0);
            if (a_ < alpha || (a_ == alpha && Code::make(kPolLb, i, t) < block)) { alpha = a_; block = Code::make(kPolLb, i, t); }
          } else if (dv > 1e-14) {
            const double a_ = fmax((UB[vi + t] - X[vi + t]) / dv, 0.0);
            if (a_ < alpha || (a_ == alpha && Code::make(kPolUb, i, t) < block)) { alpha = a_; block = Code::make(kPolUb, i, t); }
          }
        }
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          const double des = pol_quad_sum(de[ks]);
          if (h == 0 && W.shas[ks] && !sact[ks] && des > 1e-14) {
            const double a_ = fmax(cE[ks] / des, 0.0);
            if (a_ < alpha || (a_ == alpha && Code::make(kPolSess, i, ks) < block)) { alpha = a_; block = Code::make(kPolSess, i, ks); }
          }
        }
      }
      __syncthreads();
      polw_g_times(Gs, D, DU, N, Tm, Mg, tid);
      __syncthreads();
      clk.lap(4);
      // ---- (8) ... and of the site rows outside the working set -------------------------------------------------------------------
      pol_step8_rows<PolTightBytes, Code>(S, RACT, U, DU, alpha, block, tid);
      pol_block_argmin(alpha, block, RED);
      if (block < 0) alpha = 1.0;
      clk.lap(5);
      // ---- (9) move; the new multipliers; the blocking constraint joins the working set ------------------------------------------------
      double xm = 0;
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        for (int t = t0; t < t1; ++t) {
          const double xn = X[vi + t] + alpha * D[vi + t];
          X[vi + t] = xn;
          xm = fmax(xm, fabs(xn));
        }
      }
      const double step = pol_block_max(stepl, RED);
      const double xmax = pol_block_max(xm, RED);
      pol_step9_multipliers(R, NU, m, nrow, Tm, tid);
      if (block >= 0 && tid == 0) {   // (behind the barriers of the reductions above: every X of the move is written)
        const int kind = Code::kind(block), p0 = Code::p0(block), p1 = Code::p1(block);
        const size_t v = (size_t)p0 * Tm + p1;
        if (kind == kPolLb) { ST[v] |= 1; X[v] = LB[v]; }
        else if (kind == kPolUb) { ST[v] |= 2; X[v] = UB[v]; }
        else if (kind == kPolSess) SFL[p0 * 4 + p1] |= kPolwTight;
        else RACT.set(p0, p1, Tm);
      }
      __syncthreads();
      stall.update(block, step);
      const bool conv = stall.converged(block, step, xmax);
      clk.lap(6);
      if (!conv) continue;
      // ---- (10) multipliers of the whole working set: the most negative one leaves; none: verify and finish ---------------------------------
      double worst = -kPolTolDual * qn;
      int who = -1;
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        PolwSess W;
        W.load(A, b, i, iv);
        double smu[kMaxK];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) smu[ks] = iv ? SMU[si + ks] : 0.0;
        for (int t = t0; t < t1; ++t) {
          const int st = ST[vi + t];
          if ((st & 3) == 0 || (st & 4)) continue;
          double gr = pd * X[vi + t] + Q[vi + t] + RN[vi + t];
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) gr += (t >= W.soff[ks] && t < W.send[ks]) ? smu[ks] : 0.0;
          if ((st & 1) && (gr < worst || (gr == worst && who >= 0 && Code::make(kPolLb, i, t) < who))) { worst = gr; who = Code::make(kPolLb, i, t); }
          if ((st & 2) && (-gr < worst || (-gr == worst && who >= 0 && Code::make(kPolUb, i, t) < who))) { worst = -gr; who = Code::make(kPolUb, i, t); }
        }
        if (!eq && h == 0 && iv) {
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks)
            if ((SFL[si + ks] & kPolwTight) && (smu[ks] < worst || (smu[ks] == worst && who >= 0 && Code::make(kPolSess, i, ks) < who))) {
              worst = smu[ks]; who = Code::make(kPolSess, i, ks);
            }
        }
      }
      pol_step10_rows<PolTightBytes, Code>(RACT, NU, nrow, Tm, worst, who, tid);
      pol_block_argmin(worst, who, RED);
      if (who >= 0) {
        if (tid == 0) {
          const int kind = Code::kind(who), p0 = Code::p0(who), p1 = Code::p1(who);
          if (kind == kPolLb) ST[(size_t)p0 * Tm + p1] &= (unsigned char)~1;
          else if (kind == kPolUb) ST[(size_t)p0 * Tm + p1] &= (unsigned char)~2;
          else if (kind == kPolSess) SFL[p0 * 4 + p1] &= (unsigned char)~kPolwTight;
          else { RACT.clear(p0, p1, Tm); NU[p0 * Tm + p1] = 0.0; }
        }
        stall.reset();
        __syncthreads();
        continue;
      }
      // ---- KKT on the full problem, at the final x: G x again, the discs' normals from it (the step's rows carry the normals of
      // the point BEFORE the step) ------------------------------------------------------------------------------------------------------
      __syncthreads();
      polw_g_times(Gs, X, U, N, Tm, Mg, tid);
      __syncthreads();
      double pvl = 0, statl = 0;
      pol_kkt_rows(S, U, pvl, tid);
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        PolwSess W;
        W.load(A, b, i, iv);
        double smu[kMaxK];
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks) {
          smu[ks] = iv ? SMU[si + ks] : 0.0;
          double s = 0;
          for (int t = max(t0, W.soff[ks]); t < min(t1, W.send[ks]); ++t) s += X[vi + t];
          const double dd = pol_quad_sum(s) - W.scap[ks];
          if (W.shas[ks]) pvl = fmax(pvl, (eq ? fabs(dd) : dd) / fmax(1.0, fabs(W.scap[ks])));
        }
        for (int t = t0; t < t1; ++t) {
          if ((ST[vi + t] & 3) != 0) continue;
          double gr = pd * X[vi + t] + Q[vi + t];
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) gr += (t >= W.soff[ks] && t < W.send[ks]) ? smu[ks] : 0.0;
          for (int r = 0; r < nrow; ++r) {
            const double nu = NU[r * Tm + t];
            if (nu == 0.0) continue;
            const int j = S.row_j(r);
            if (S.is_disc(r)) {
              const double u0 = U[j * Tm + t], u1 = U[(j + M) * Tm + t], val = hypot(u0, u1);
              gr += nu * (u0 * Gs[(size_t)j * N + i] + u1 * Gs[(size_t)(j + M) * N + i]) / val;
            } else {
              gr += nu * Gs[(size_t)j * N + i];
            }
          }
          statl = fmax(statl, fabs(gr));
        }
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
    if (success) {
      double ol = 0;
      for (int i0 = 0; i0 < N; i0 += 64) {
        POLW_TILE(i0);
        for (int t = t0; t < t1; ++t) {
          const double xx = X[vi + t];
          A.x[((size_t)b * N + i) * Tm + t] = xx;
          ol += (0.5 * pd_user * xx + Q[vi + t]) * xx;
        }
      }
      pol_results(A, S, NU, U, true, ol, rounds, why, prim_out, stat_out, RED, tid);
    } else {
      // a polish that gives up leaves the problem as the solver left it (the restore kernel gives its status back)
      if (tid == 0) atomicAdd(A.stats + why, 1);
      __syncthreads();
    }
  }
#undef POLW_TILE
}

}  // namespace acnqp
