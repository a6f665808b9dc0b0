// Gradients through the solve (acnqp_vjp_device / acnqp_vjp_host, include/acn_qp.h): for an answer (x, y)
// and the caller's g = dL/dx, the adjoint of the solution map -- dL/dq, dL/dcap, dL/d(site limit), dL/dlb, dL/dub -- by ONE
// solve with the KKT matrix of the optimal working set.  That matrix is the one a Newton round of polish_kernel
// (acn_qp_polish.hpp) factorises; it is symmetric, so the adjoint system
//     H a + C'm = g_free,   C a = 0          (H = pd I + the discs' curvature, C = the tight rows on the free variables)
// is that round with g in place of pd x + q and zero constraint residuals: its step is dx = -a, its multipliers are -m.
// With the Newton system K [dx; dm] = [-dq; dc] of a perturbed KKT point, g'dx = [a; m]' K [dx; dm] = -a'dq + m'dc:
//     dL/dq = -a,   dL/dcap_s = m_s,   dL/dlim_(r, t) = m_(r, t),
// and a variable fixed at a bound enters the free equations as a known column, dL/dbound = g - (H a + C'm) at that variable.
//
// One workgroup of 256 threads per problem, thread layout, LDS carve-up (PolishLds) and steps 1 ... 7 as polish_kernel's for
// the same shapes (N <= 64, horizons <= 32, K <= 4, no flat or max row): the per-thread phases are written out here, every
// step on the LDS tables is a call into acn_qp_polish_steps.hpp.  No ratio test, no queue, no statistics.  The working set
// is the polish's first guess at (x, y), with the polish's thresholds.
//
// Determinism: every sum runs in a fixed order (a thread's own periods, a quad's two exchanges, a table row's loop);
// workgroups share nothing and no floating-point atomic is used: the same problem gives the same bits in any batch and at
// any position.  tests/vjp_spec.py restates the system densely in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acn_qp_common.hpp"
#include "acn_qp_polish_steps.hpp"

namespace acnqp {

constexpr int kVjpDone = 0, kVjpStatus = 1, kVjpRows = 2, kVjpPivot = 3;   // info[0]

struct VjpArgs {
  int B, N, Tm, K, M, Mg, cone, has_peak;
  int max_rows, blk_doubles, max_sess;   // the tables of PolishLds, as the polish sizes them (vjp_tables)
  const double *G, *limits;              // acnqp_site.G [Mg][N] and limits [M] as the caller gave them
  const int32_t* horizon;
  const double *lb, *ub, *q, *pdiag;
  const int32_t *s_off, *s_len;
  const double* s_cap;
  const uint8_t* s_eq;
  const double* peak;
  const double *x, *y;                   // the point; y is not read on a site without rows
  const int32_t* status;                 // or nullptr: all solved
  const double* gx;                      // dL/dx [B][N][Tm]
  double *gq, *gcap, *grow, *glb, *gub;  // glb, gub may be nullptr
  int32_t* info;                         // [B][4]
  double* res;                           // [B][2]
  double reg_rel;
};

// exact zeros in every gradient of problem b, the verdict, no counts, no residuals
__device__ inline void vjp_give_up(const VjpArgs& A, int b, int nrow, int verdict, int tid) {
  const size_t n = (size_t)A.N * A.Tm;
  for (size_t k = tid; k < n; k += kPolThreads) {
    A.gq[(size_t)b * n + k] = 0.0;
    if (A.glb) A.glb[(size_t)b * n + k] = 0.0;
    if (A.gub) A.gub[(size_t)b * n + k] = 0.0;
  }
  for (int k = tid; k < A.K * A.N; k += kPolThreads) A.gcap[(size_t)b * A.K * A.N + k] = 0.0;
  for (int k = tid; k < nrow * A.Tm; k += kPolThreads) A.grow[(size_t)b * nrow * A.Tm + k] = 0.0;
  if (tid < 4) A.info[(size_t)b * 4 + tid] = tid == 0 ? verdict : 0;
  if (tid < 2) A.res[(size_t)b * 2 + tid] = 0.0;
}

template <int kPolTQ>
__global__ __launch_bounds__(kPolThreads, kPolTQ == 4 ? 2 : 1) void vjp_kernel(const VjpArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vjp_smem[];
  double* sm = reinterpret_cast<double*>(vjp_smem);
  const int N = A.N, Tm = A.Tm, K = A.K, M = A.M, Mg = A.Mg;
  const bool soc = A.cone == 1;
  const int nrow = M + (A.has_peak ? 1 : 0);
  const PolishLds L(N, Tm, Mg, nrow, A.max_rows, A.blk_doubles, A.max_sess);
  const int MS = A.max_sess;
  double *Xs = sm + L.xs, *Ds = sm + L.ds, *Gs = sm + L.gs, *U = sm + L.u, *Ys = sm + L.du, *NU = sm + L.nu;   // (Ys: y of the problem, where the polish keeps G dx)
  double *RC0 = sm + L.rc0, *RC1 = sm + L.rc1, *RCA = sm + L.rca, *RDG = sm + L.rdg, *LAM = sm + L.lam, *RED = sm + L.red;
  double *BLK = sm + L.blk, *CAP = sm + L.cap, *ZB = sm + L.zb, *ZV = sm + L.zv, *SISQ = sm + L.sisq;
  int* RJ = reinterpret_cast<int*>(sm + L.ints);
  int* RR = RJ + A.max_rows;
  int* RT = RR + A.max_rows;
  int* TSTART = RT + A.max_rows;
  int* BOFF = TSTART + Tm + 1;
  const PolTightMask RACT{reinterpret_cast<unsigned*>(BOFF + Tm + 1)};
  int* MISC = reinterpret_cast<int*>(RACT.w + nrow);   // [2] session columns, [3] bad pivot
  int* SI = MISC + 8;
  int* SKS = SI + MS;
  signed char* CS = reinterpret_cast<signed char*>(SKS + MS);   // per (i, t): -2 not free, -1 free, k >= 0 free in tight session k
  const PolRows R{RJ, RR, RT, RC0, RC1, RCA, RDG, LAM};

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int i = tid >> 2, h = tid & 3;
  const int TQ = (Tm + 3) >> 2;
  const bool iv = i < N;
  const size_t n = (size_t)N * Tm;

  const int st = A.status ? A.status[b] : 1;
  if (st != 1 && st != 5) { vjp_give_up(A, b, nrow, kVjpStatus, tid); return; }   // neither SOLVED nor SOLVED_INACCURATE (block-uniform)
  const PolSite S{N, Tm, M, Mg, nrow, b, soc, A.limits, A.peak};
  const bool eq = A.s_eq[b] != 0;
  const int T = A.horizon[b];

  // ---- own variables: the polish's first working set at x; g = dL/dx on the periods of the horizon ------------------------
  double xv[kPolTQ], lbv[kPolTQ], ubv[kPolTQ], qv[kPolTQ], gxv[kPolTQ], dv[kPolTQ], gv[kPolTQ];
  unsigned atlb = 0, atub = 0, fixedm = 0, validm = 0, livem = 0;
  double qmax = 0, umax = 0, gmax = 0;
#pragma unroll
  for (int k = 0; k < kPolTQ; ++k) {
    const int t = h * TQ + k;
    const bool ok = iv && k < TQ && t < Tm;
    const bool live = ok && t < T;
    const size_t idx = ((size_t)b * N + (ok ? i : 0)) * Tm + (ok ? t : 0);
    lbv[k] = ok ? A.lb[idx] : 0.0;
    ubv[k] = ok ? fmax(A.ub[idx], lbv[k]) : 0.0;
    qv[k] = ok ? A.q[idx] : 0.0;
    xv[k] = ok ? fmin(fmax(A.x[idx], lbv[k]), ubv[k]) : 0.0;
    gxv[k] = live ? A.gx[idx] : 0.0;
    dv[k] = 0; gv[k] = 0;
    validm |= ok ? 1u << k : 0u;
    livem |= live ? 1u << k : 0u;
    qmax = fmax(qmax, fabs(qv[k]));
    umax = fmax(umax, ubv[k]);
    gmax = fmax(gmax, fabs(gxv[k]));
    const bool lo = xv[k] <= lbv[k] + kPolTolBound;
    const bool hi = xv[k] >= ubv[k] - kPolTolBound && !lo;
    atlb |= lo ? 1u << k : 0u;
    atub |= hi ? 1u << k : 0u;
    fixedm |= (ubv[k] - lbv[k] <= kPolTolBound) ? 1u << k : 0u;
  }
  const double qraw = pol_block_max(qmax, RED);
  const double ubmax = pol_block_max(umax, RED);
  const double gnorm = fmax(1.0, pol_block_max(gmax, RED));
  const double qn = fmax(1.0, qraw);
  const double pd = effective_pdiag<double>(A.pdiag[b], A.reg_rel, qraw, ubmax, T, false);
  const unsigned freem = validm & ~(atlb | atub);
  // ---- own sessions (the same on the four threads of the quad) ---------------------------------------------------------------
  unsigned swm[kMaxK];      // bit k: own period k lies in the window
  double scap[kMaxK], smu[kMaxK], nfree[kMaxK];
  bool son[kMaxK];          // the energy row is tight and has free variables: a row of C
#pragma unroll
  for (int ks = 0; ks < kMaxK; ++ks) {
    swm[ks] = 0; scap[ks] = 0; smu[ks] = 0;
    bool has = false;
    if (ks < K && iv) {
      const size_t sidx = ((size_t)b * K + ks) * N + i;
      const int off = A.s_off[sidx], len = A.s_len[sidx];
      scap[ks] = A.s_cap[sidx];
      has = len > 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        const int t = h * TQ + k;
        if (k < TQ && t >= off && t < off + len && t < Tm) swm[ks] |= 1u << k;
      }
    }
    double s = 0, nf = 0;
#pragma unroll
    for (int k = 0; k < kPolTQ; ++k) {
      const bool inw = (swm[ks] >> k) & 1u;
      s += inw ? xv[k] : 0.0;
      nf += (inw && ((freem >> k) & 1u)) ? 1.0 : 0.0;
    }
    s = pol_quad_sum(s);
    nfree[ks] = pol_quad_sum(nf);
    const bool act = has && (eq || s >= scap[ks] - kPolTolBound * fmax(1.0, fabs(scap[ks])));
    son[ks] = act && nfree[ks] > 0;
  }
  // ---- site data; the tight site rows by their multipliers in y ---------------------------------------------------------------
  for (int k = tid; k < Mg * N; k += kPolThreads) Gs[k] = A.G[k];
  for (int k = tid; k < Mg * Tm; k += kPolThreads) Ys[k] = A.y[(size_t)b * Mg * Tm + k];
  if (nrow == 0)   // (pol_step3_rows states where a period's rows start through its site row 0)
    for (int t = tid; t <= Tm; t += kPolThreads) TSTART[t] = 0;
  pol_first_guess(S, RACT, A.y, NU, qn, tid);
  // ---- (1) x mirror, which session a free variable belongs to -----------------------------------------------------------------
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
  // ---- (2) G x ----------------------------------------------------------------------------------------------------------------
  pol_g_times<int>(Gs, Xs, U, N, Tm, Mg, tid);
  __syncthreads();
  // ---- (3) rows and session columns of the Schur system -----------------------------------------------------------------------
  pol_step3_rows(S, RACT, R, U, NU, TSTART, A.max_rows, qn, pd, RED, tid);
  pol_step3_columns(son, nfree, h == 0 && iv, i, MS, SI, SKS, SISQ, MISC + 2, RED, [](int, int) {});
  // ---- (4) v_free = -P g: the caller's g in place of pd x + q, c_E = 0 ---------------------------------------------------------
  double Eg[kMaxK];
#pragma unroll
  for (int k = 0; k < kPolTQ; ++k) gv[k] = ((freem >> k) & 1u) ? gxv[k] : 0.0;
#pragma unroll
  for (int ks = 0; ks < kMaxK; ++ks) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < kPolTQ; ++k) s += (((swm[ks] & freem) >> k) & 1u) ? gv[k] : 0.0;
    Eg[ks] = pol_quad_sum(s);
  }
#pragma unroll
  for (int k = 0; k < kPolTQ; ++k) {
    double pg = gv[k];
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) pg -= (son[ks] && (((swm[ks] & freem) >> k) & 1u)) ? Eg[ks] / nfree[ks] : 0.0;
    const int t = h * TQ + k;
    if (iv && k < TQ && t < Tm) Ds[i * Tm + t] = -pg;
  }
  __syncthreads();
  const int m = TSTART[Tm], nsa = MISC[2];
  if (m > A.max_rows || nsa > MS) { vjp_give_up(A, b, nrow, kVjpRows, tid); return; }   // (block-uniform)
  for (int a = tid; a < m; a += kPolThreads) RCA[a] = 0.0;   // c_A = 0
  if (tid == 0) { pol_block_offsets(TSTART, BOFF, Tm); MISC[3] = 0; }
  __syncthreads();
  const int E = BOFF[Tm];
  if (E > A.blk_doubles) { vjp_give_up(A, b, nrow, kVjpRows, tid); return; }
  // ---- (5), (6) the Schur system, with the polish's dual regularisation ----------------------------------------------------------
  pol_step5<int>(R, Gs, Ds, CS, TSTART, BOFF, BLK, CAP, N, Tm, M, m, E, nsa, pd, RED, tid);
  if (!pol_step6_lds(R, Gs, CS, TSTART, BOFF, BLK, CAP, ZB, ZV, SISQ, SI, SKS, MISC + 3, N, Tm, M, m, nsa, MS, tid)) {
    vjp_give_up(A, b, nrow, kVjpPivot, tid);
    return;
  }
  // ---- (7) the step dx = -a and the multipliers -m ------------------------------------------------------------------------------
  double rl[kPolTQ];   // (R' lam)(i, t), on every variable: at a fixed one it is the column's image under the site rows and the curvature
#pragma unroll
  for (int k = 0; k < kPolTQ; ++k) {
    rl[k] = 0;
    const int t = h * TQ + k;
    if (iv && k < TQ && t < Tm) {
      for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) {
        const int ja = RJ[a];
        const double c1 = RC1[a];
        const double ra = RC0[a] * Gs[ja * N + i] + (c1 != 0.0 ? c1 * Gs[(ja + M) * N + i] : 0.0);
        rl[k] += LAM[a] * ra;
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
    smu[ks] = son[ks] ? -Ev[ks] / nfree[ks] : 0.0;
  }
  double r0l = 0;   // |H a + C'm - g| on the free variables, with the multipliers as solved
#pragma unroll
  for (int k = 0; k < kPolTQ; ++k) {
    double pv = gv[k] + rl[k], ms = 0;
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      pv -= (son[ks] && (((swm[ks] & freem) >> k) & 1u)) ? Ev[ks] / nfree[ks] : 0.0;
      ms += ((swm[ks] >> k) & 1u) ? smu[ks] : 0.0;
    }
    const bool fr = (freem >> k) & 1u;
    dv[k] = fr ? -pv / pd : 0.0;
    r0l = fmax(r0l, fr ? fabs(pd * dv[k] + gv[k] + rl[k] + ms) : 0.0);
    gv[k] = gxv[k] + rl[k] + ms;   // from here: g - (H a + C'm) at a fixed variable
  }
  // ---- the primal point's own multipliers: mu and z from stationarity, for the weak members and the second residual --------------
  double r1l = 0, nweak = 0, nfr = 0;
  {
    double rp[kPolTQ], mp[kMaxK];
#pragma unroll
    for (int k = 0; k < kPolTQ; ++k) {
      const int t = h * TQ + k;
      double acc = 0;
      if (iv && k < TQ && t < Tm)
        for (int j = 0; j < Mg; ++j) acc += Gs[j * N + i] * Ys[j * Tm + t];
      rp[k] = pd * xv[k] + qv[k] + acc;
    }
#pragma unroll
    for (int ks = 0; ks < kMaxK; ++ks) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) s += (((swm[ks] & freem) >> k) & 1u) ? rp[k] : 0.0;
      s = pol_quad_sum(s);
      mp[ks] = son[ks] ? -s / nfree[ks] : 0.0;
      if (h == 0 && !eq && son[ks] && fabs(mp[ks]) < kPolTolDual * qn) nweak += 1.0;
    }
#pragma unroll
    for (int k = 0; k < kPolTQ; ++k) {
      double z = rp[k];
#pragma unroll
      for (int ks = 0; ks < kMaxK; ++ks) z += ((swm[ks] >> k) & 1u) ? mp[ks] : 0.0;
      if ((freem >> k) & 1u) { r1l = fmax(r1l, fabs(z)); nfr += 1.0; }
      else if (((validm & ~fixedm) >> k) & 1u) nweak += fabs(z) < kPolTolDual * qn ? 1.0 : 0.0;
    }
    // (a tight site row is never weak: it is tight because its multiplier exceeds kPolTolRow qn = kPolTolDual qn)
  }
  const double res0 = pol_block_max(r0l, RED) / gnorm;
  const double res1 = pol_block_max(r1l, RED) / qn;
  const double weak = pol_block_sum(nweak, RED);
  const double nfr_all = pol_block_sum(nfr, RED);
  pol_step9_multipliers(R, NU, m, nrow, Tm, tid);   // NU: the multipliers of the normal rows, zero elsewhere
  __syncthreads();
  // ---- results ---------------------------------------------------------------------------------------------------------------------
#pragma unroll
  for (int k = 0; k < kPolTQ; ++k) {
    const int t = h * TQ + k;
    if (!(iv && k < TQ && t < Tm)) continue;
    const size_t idx = ((size_t)b * N + i) * Tm + t;
    const bool live = (livem >> k) & 1u, fr = (freem >> k) & 1u;
    A.gq[idx] = live && fr ? dv[k] : 0.0;
    if (A.glb) A.glb[idx] = live && ((atlb >> k) & 1u) ? gv[k] : 0.0;
    if (A.gub) A.gub[idx] = live && ((atub >> k) & 1u) ? gv[k] : 0.0;
  }
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

// the tables of a shape, sized as the polish sizes them for a workgroup that has the CU's LDS to itself; false: not even one
// period's full block fits
struct VjpTables { int max_rows, max_sess, blk_doubles; };
bool vjp_tables(int N, int Tm, int K, int Mg, int nrow, VjpTables* t);
hipError_t launch_vjp(const VjpArgs& a, hipStream_t st);
// the long-horizon kernel (acn_qp_vjp_long.hpp: horizons 33 ... 288, the state in a slab of global memory per workgroup):
// workgroups (slabs) of a launch -- one per problem up to the device's compute units, fewer where the slabs would pass
// kVjpLongScratchBytes -- and the launcher (slab: that many slabs of PolishLongLayout::slab_bytes(); max_rows, max_sess,
// blk_doubles of `a`: the layout's worst case)
int vjp_long_grid(int N, int Tm, int K, int Mg, int nrow, int batch, int cus);
hipError_t launch_vjp_long(const VjpArgs& a, double* slab, int grid, hipStream_t st);

}  // namespace acnqp
