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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acn_qp_common.hpp"
#include "acn_qp_polclaim.hpp"

namespace acnqp {

constexpr int kPolThreads = 256;
constexpr int kPolMaxRounds = 96;
constexpr int kPolMaxRows = 256;      // rows of the Schur system at most (row tables; one thread per row in the triangular solves)
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

constexpr int kPolMaxSess = 128;      // tight sessions with free variables (columns of V) at most (PolishArgs.max_sess <= this)

// LDS carve-up in doubles (host: size; device: offsets)
struct PolishLds {
  int xs, ds, gs, u, du, nu, invn, rc0, rc1, rca, rdg, lam, blk, cap, zb, zv, sisq, red, ints, total;
  int mt_max;   // rows of one period's block at most: two per site row
  __host__ __device__ PolishLds(int N, int Tm, int Mg, int nrow, int max_rows, int blk_doubles, int max_sess) {
    int o = 0;
    mt_max = 2 * nrow;
    xs = o; o += N * Tm;
    ds = o; o += N * Tm;
    gs = o; o += Mg * N;
    u = o; o += Mg * Tm;
    du = o; o += Mg * Tm;
    nu = o; o += nrow * Tm;
    invn = o; o += N * 4;
    rc0 = o; o += max_rows;
    rc1 = o; o += max_rows;
    rca = o; o += max_rows;
    rdg = o; o += max_rows;
    lam = o; o += max_rows;
    blk = o; o += blk_doubles;                               // the per-period blocks of B, packed lower, one after the other
    cap = o; o += max_sess * (max_sess + 1) / 2;             // C = I - V' B^-1 V, packed lower
    zb = o; o += mt_max * max_sess;                          // L_t^-1 V_t of the block in work
    zv = o; o += max_sess;                                   // V' y, then w
    sisq = o; o += max_sess;                                 // 1 / sqrt(n_s) of the session columns
    red = o; o += 16;
    ints = o;   // ints from here: rj, rr, rt [max_rows], tstart[Tm + 1], boff[Tm + 1], ract[nrow], misc[8], si / sks [max_sess]; then cs[N * Tm] bytes
    const int nint = 3 * max_rows + 2 * (Tm + 1) + nrow + 8 + 2 * max_sess;
    o += (nint + 1) / 2 + (N * Tm + 7) / 8;
    total = o;
  }
  // doubles for the blocks that fit `bytes` of LDS, at most what the worst case needs (every site row tight in every period)
  __host__ static int blocks_that_fit(int N, int Tm, int Mg, int nrow, int max_rows, int max_sess, int bytes) {
    const int worst = Tm * (2 * nrow) * (2 * nrow + 1) / 2;
    const long long fixed = (long long)PolishLds(N, Tm, Mg, nrow, max_rows, 0, max_sess).total * 8;
    const long long room = ((long long)bytes - fixed) / 8;
    return (int)(room < 0 ? 0 : (room < worst ? room : worst));
  }
};

// LDS traffic inside ONE wave: writes of some lanes read by others in the next step (the tiled kernel's idiom)
__device__ inline void pol_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// B_t^-1 applied in place to the rows [a0, a0 + mt) of the LDS vector `v`, by ONE wave: blk = the block's packed L D L'
// (L unscaled, acn_qp_polish.hpp phase 6a), dinv = 1 / D of its rows.
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

// blocking-constraint / release codes: kind in the top bits
constexpr int kPolLb = 0, kPolUb = 1, kPolSess = 2, kPolRow = 3;
__device__ inline int pol_code(int kind, int p0, int p1) { return (kind << 24) | (p0 << 8) | p1; }

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
  unsigned* RACT = reinterpret_cast<unsigned*>(BOFF + Tm + 1);   // per site row: bit t = tight at period t
  int* MISC = reinterpret_cast<int*>(RACT + nrow);     // [0] m, [1] fail flag, [2] session columns, [3] bad pivot
  int* SI = MISC + 8;                                  // session columns of V: EVSE, slot
  int* SKS = SI + MS;
  signed char* CS = reinterpret_cast<signed char*>(SKS + MS);   // per (i, t): -2 not free, -1 free, k >= 0 free in tight session k
  __shared__ int q_slot;

  const int tid = threadIdx.x;
  const int i = tid >> 2, h = tid & 3;
  const int TQ = (Tm + 3) >> 2;
  const bool iv = i < N;
  auto row_j = [&](int r) { return r < M ? r : Mg - 1; };
  auto row_is_disc = [&](int r) { return soc && r < M; };

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
      const int nlist = *A.count;
      pos = queue_next(A.queue, nlist < A.B ? nlist : A.B, q_round, &q_slot);
      if (pos < 0) break;
      b = A.list[pos];
    }
    if (A.status[b] != kStatusPolish) continue;   // (block-uniform)
    if (tid == 0) atomicAdd(A.stats + 0, 1);
    if (tid == 0 && A.alongside) atomicAdd(A.taken, 1);
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
    for (int r = tid; r < nrow; r += kPolThreads) RACT[r] = 0;
    __syncthreads();
    for (int k = tid; k < nrow * Tm; k += kPolThreads) {
      const int r = k / Tm, t = k - r * Tm, j = row_j(r);
      const double y0 = A.y[((size_t)b * Mg + j) * Tm + t];
      const double mag = row_is_disc(r) ? hypot(y0, A.y[((size_t)b * Mg + j + M) * Tm + t]) : y0;
      const double lim = r < M ? A.limits[r] : A.peak[(size_t)b * Tm + t];
      const bool on = mag > kPolTolRow * qn && lim < 1e299;
      NU[k] = on ? mag : 0.0;
      if (on) atomicOr(&RACT[r], 1u << t);
    }
    __syncthreads();

    int why = 4, rounds = 0;   // reason of a failure (index into stats), rounds made
    int stall = 0;             // full steps in a row without progress (noise floor)
    double best_step = 1e300;
    // coarse phase clock (thread 0, 100 MHz ticks summed into stats[8 + phase]): where a polish spends its time
    unsigned long long tick = wall_clock64();
    unsigned tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define POL_TICK(ph) do { const unsigned long long _n = wall_clock64(); tacc[ph] += (unsigned)(_n - tick); tick = _n; } while (0)
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
      for (int k = tid; k < Mg * Tm; k += kPolThreads) {
        const int j = k / Tm, t = k - j * Tm;
        double s = 0;
        for (int e = 0; e < N; ++e) s += Gs[j * N + e] * Xs[e * Tm + t];
        U[k] = s;
      }
      __syncthreads();
      // ---- (3) rows of the Schur system, period-major: pair k = t nrow + r of (period, site row) -> 0 / 1 / 2 rows (a tight
      // disc: its normal row and, with a multiplier worth it, its tangent row); offsets by a block-wide exclusive scan
      {
        int base = 0;
        bool over = false;
        for (int k0 = 0; k0 < nrow * Tm; k0 += kPolThreads) {
          const int k = k0 + tid;
          const bool in = k < nrow * Tm;
          const int t = in ? k / nrow : 0, r = in ? k - t * nrow : 0, j = row_j(r);
          int need = 0;
          double lim = 0, u0 = 0, u1 = 0, val = 0, nu = 0;
          if (in && ((RACT[r] >> t) & 1u)) {
            lim = r < M ? A.limits[r] : A.peak[(size_t)b * Tm + t];
            if (row_is_disc(r)) {
              u0 = U[j * Tm + t]; u1 = U[(j + M) * Tm + t];
              val = hypot(u0, u1);
              nu = NU[r * Tm + t];
              need = val > 1e-12 ? (nu > kPolTangentMin * qn ? 2 : 1) : 0;
            } else {
              need = 1;
            }
          }
          int incl = need;
          for (int o = 1; o < 64; o <<= 1) { const int nb = __shfl_up(incl, o); incl += (tid & 63) >= o ? nb : 0; }
          int* WT = reinterpret_cast<int*>(RED);
          __syncthreads();
          if ((tid & 63) == 63) WT[tid >> 6] = incl;
          __syncthreads();
          int before = base;
          for (int w = 0; w < (tid >> 6); ++w) before += WT[w];
          const int total = WT[0] + WT[1] + WT[2] + WT[3];
          const int m0 = before + incl - need;
          if (in && r == 0) TSTART[t] = m0;
          if (base + total > A.max_rows) { over = true; break; }   // (block-uniform)
          if (need >= 1) {
            if (row_is_disc(r)) {
              const double n0 = u0 / val, n1 = u1 / val;
              RJ[m0] = j; RR[m0] = r; RT[m0] = t; RC0[m0] = n0; RC1[m0] = n1; RCA[m0] = lim - val; RDG[m0] = 0.0;
              if (need == 2) {
                RJ[m0 + 1] = j; RR[m0 + 1] = -1 - r; RT[m0 + 1] = t; RC0[m0 + 1] = -n1; RC1[m0 + 1] = n0; RCA[m0 + 1] = 0.0;
                RDG[m0 + 1] = pd * val / nu;
              }
            } else {
              RJ[m0] = j; RR[m0] = r; RT[m0] = t; RC0[m0] = 1.0; RC1[m0] = 0.0; RCA[m0] = lim - U[j * Tm + t]; RDG[m0] = 0.0;
            }
          }
          base += total;
        }
        if (tid == 0) { TSTART[Tm] = base; MISC[0] = base; MISC[1] = over ? 1 : 0; }
        // session columns of V: the tight sessions with free variables, in (EVSE, slot) order (same scan)
        int cnt = 0;
        if (h == 0 && iv) {
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks) cnt += son[ks] ? 1 : 0;
        }
        int incl = cnt;
        for (int o = 1; o < 64; o <<= 1) { const int nb = __shfl_up(incl, o); incl += (tid & 63) >= o ? nb : 0; }
        int* WT = reinterpret_cast<int*>(RED);
        __syncthreads();
        if ((tid & 63) == 63) WT[tid >> 6] = incl;
        __syncthreads();
        int pos = incl - cnt;
        for (int w = 0; w < (tid >> 6); ++w) pos += WT[w];
        if (tid == 0) MISC[2] = WT[0] + WT[1] + WT[2] + WT[3];
        if (h == 0 && iv) {
#pragma unroll
          for (int ks = 0; ks < kMaxK; ++ks)
            if (son[ks]) {
              if (pos < MS) { SI[pos] = i; SKS[pos] = ks; SISQ[pos] = 1.0 / sqrt(nfree[ks]); }
              ++pos;
            }
        }
      }
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
      const int m = MISC[0], nsa = MISC[2];
      if (MISC[1] || nsa > MS) { why = 2; break; }
      if (tid == 0) {   // packed blocks of B, one per period, one after the other
        int o = 0;
        for (int t = 0; t < Tm; ++t) { BOFF[t] = o; const int mt = TSTART[t + 1] - TSTART[t]; o += mt * (mt + 1) / 2; }
        BOFF[Tm] = o;
        MISC[3] = 0;
      }
      __syncthreads();
      const int E = BOFF[Tm];
      if (E > A.blk_doubles) { why = 2; break; }
      POL_TICK(0);
      // R_a at EVSE e (a row lives on its own period's variables)
      auto row_at = [&](int a_, int e_) __attribute__((always_inline)) -> double {
        const int ja = RJ[a_];
        const double c1 = RC1[a_];
        return RC0[a_] * Gs[ja * N + e_] + (c1 != 0.0 ? c1 * Gs[(ja + M) * N + e_] : 0.0);
      };
      // ---- (5) rhs = R v_free - pd c_A;  B = R R' + diag + reg I, BLOCK DIAGONAL by period;  C = I ---------------------------
      // (R P R' + diag + reg I) lam = rhs with R P R' = R R' - V V', V[:, s] = R 1_s / sqrt(n_s) over the tight sessions with free
      // variables: Woodbury -- lam = y + B^-1 V w, y = B^-1 rhs, (I - V' B^-1 V) w = V' y.  Per-period L D L' factors of <= 2 nrow
      // rows and one of the size of the tight sessions, instead of one dense factorisation of the size of ALL tight site rows:
      // the 200-row systems of the horizon-24 stragglers fit, and a round costs what its blocks cost (oracle/polish_ref.py).
      double dloc = 0;
      for (int a = tid; a < m; a += kPolThreads) {
        const int ta = RT[a];
        const double* g0 = Gs + RJ[a] * N;          // (the row's constants once, not once per EVSE: this loop and the block
        const double* g1 = g0 + M * N;              //  build below were 20 us of a 79 us round as chains of LDS reads)
        const double c0 = RC0[a], c1 = RC1[a];
        const bool two = c1 != 0.0;
        double sacc = 0, d2 = 0;
        for (int e = 0; e < N; ++e) {
          const double ra = c0 * g0[e] + (two ? c1 * g1[e] : 0.0);
          sacc += ra * Ds[e * Tm + ta];
          d2 += CS[e * Tm + ta] != -2 ? ra * ra : 0.0;
        }
        LAM[a] = sacc - pd * RCA[a];
        dloc = fmax(dloc, d2);
      }
      const double reg = fmax(kPolRegRel * pd, kPolRegDiag * pol_block_max(dloc, RED));
      {
        int t = 0;
        for (int p = tid; p < E; p += kPolThreads) {
          while (BOFF[t + 1] <= p) ++t;
          const int q_ = p - BOFF[t];
          int ar = (int)((sqrt(8.0 * (double)q_ + 1.0) - 1.0) * 0.5);
          while ((ar + 1) * (ar + 2) / 2 <= q_) ++ar;
          while (ar * (ar + 1) / 2 > q_) --ar;
          const int cr = q_ - ar * (ar + 1) / 2;
          const int a = TSTART[t] + ar, c = TSTART[t] + cr;
          const double *ga0 = Gs + RJ[a] * N, *ga1 = ga0 + M * N, *gc0 = Gs + RJ[c] * N, *gc1 = gc0 + M * N;
          const double a0c = RC0[a], a1c = RC1[a], c0c = RC0[c], c1c = RC1[c];
          const bool atwo = a1c != 0.0, ctwo = c1c != 0.0;
          double sacc = 0;
          for (int e = 0; e < N; ++e) {
            const double ra = a0c * ga0[e] + (atwo ? a1c * ga1[e] : 0.0);
            const double rc = c0c * gc0[e] + (ctwo ? c1c * gc1[e] : 0.0);
            sacc += CS[e * Tm + t] != -2 ? ra * rc : 0.0;
          }
          BLK[p] = sacc + (a == c ? RDG[a] + reg : 0.0);
        }
      }
      for (int p = tid; p < nsa * (nsa + 1) / 2; p += kPolThreads) CAP[p] = 0.0;
      __syncthreads();
      for (int c = tid; c < nsa; c += kPolThreads) CAP[c * (c + 1) / 2 + c] = 1.0;
      POL_TICK(1);
      // ---- (6a) L D L' of every block, a wave per block (unit lower L stored unscaled, 1 / D in RDG) ------------------------------
      const int wave_ = tid >> 6, lane_ = tid & 63;
      for (int t = wave_; t < Tm; t += 4) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        double* blk = BLK + BOFF[t];
        bool bad = false;
        for (int k = 0; k < mt && !bad; ++k) {
          const double piv = blk[k * (k + 1) / 2 + k];
          if (!(piv > 0.0)) { bad = true; break; }   // (wave-uniform)
          const double pinv = 1.0 / piv;
          for (int rr = k + 1 + (lane_ >> 3); rr < mt; rr += 8) {
            const double lr = blk[rr * (rr + 1) / 2 + k] * pinv;
            for (int c = k + 1 + (lane_ & 7); c <= rr; c += 8) blk[rr * (rr + 1) / 2 + c] -= lr * blk[c * (c + 1) / 2 + k];
          }
          pol_wave_sync();
        }
        if (bad) { if (lane_ == 0) MISC[3] = 1; continue; }
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
            for (int a = TSTART[t]; a < TSTART[t + 1]; ++a) z += row_at(a, ic) * LAM[a];
        ZV[c] = z * SISQ[c];
      }
      for (int t = 0; t < Tm; ++t) {
        const int mt = TSTART[t + 1] - TSTART[t], a0 = TSTART[t];
        if (mt == 0) continue;   // (block-uniform)
        const double* blk = BLK + BOFF[t];
        for (int idx = tid; idx < mt * nsa; idx += kPolThreads) {
          const int k = idx / nsa, c = idx - k * nsa;
          const int ic = SI[c];
          ZB[k * MS + c] = CS[ic * Tm + t] == SKS[c] ? row_at(a0 + k, ic) * SISQ[c] : 0.0;
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
          int c = (int)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
          while ((c + 1) * (c + 2) / 2 <= p) ++c;
          while (c * (c + 1) / 2 > p) --c;
          const int c2 = p - c * (c + 1) / 2;
          if (CS[SI[c] * Tm + t] != SKS[c] || CS[SI[c2] * Tm + t] != SKS[c2]) continue;
          double sacc = 0;
          for (int k = 0; k < mt; ++k) sacc += ZB[k * MS + c] * RDG[a0 + k] * ZB[k * MS + c2];
          CAP[p] -= sacc;
        }
        __syncthreads();
      }
      POL_TICK(2);
      // ---- (6d) C = L D L' (packed, one barrier per column), C w = V' y ----------------------------------------------------------------
      bool bad_pivot = false;
      for (int k = 0; k < nsa; ++k) {
        __syncthreads();
        const double piv = CAP[k * (k + 1) / 2 + k];
        if (!(piv > 0.0)) { bad_pivot = true; break; }   // (uniform: every thread reads the same entry)
        const double pinv = 1.0 / piv;
        for (int rr = k + 1 + (tid >> 4); rr < nsa; rr += 16) {
          const double lr = CAP[rr * (rr + 1) / 2 + k] * pinv;
          double* row = CAP + rr * (rr + 1) / 2;
          for (int c = k + 1 + (tid & 15); c <= rr; c += 16) row[c] -= lr * CAP[c * (c + 1) / 2 + k];
        }
      }
      if (bad_pivot) { why = 3; break; }
      {
        __syncthreads();
        double* DI = ZB;   // 1 / D of C (the Z buffer is free now)
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
      }
      // ---- (6e) lam = y + B^-1 (V w) ---------------------------------------------------------------------------------------------------
      for (int a = tid; a < m; a += kPolThreads) {
        const int ta = RT[a];
        double sacc = 0;
        for (int c = 0; c < nsa; ++c) {
          const int ic = SI[c];
          if (CS[ic * Tm + ta] == SKS[c]) sacc += row_at(a, ic) * SISQ[c] * ZV[c];
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
      POL_TICK(3);
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
      for (int k = tid; k < Mg * Tm; k += kPolThreads) {
        const int j = k / Tm, t = k - j * Tm;
        double s = 0;
        for (int e = 0; e < N; ++e) s += Gs[j * N + e] * Ds[e * Tm + t];
        DU[k] = s;
      }
      __syncthreads();
      POL_TICK(4);
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
          if (a_ < alpha) { alpha = a_; block = pol_code(kPolLb, i, t); }
        } else if (d > 1e-14) {
          const double a_ = fmax((ubv[k] - xv[k]) / d, 0.0);
          if (a_ < alpha) { alpha = a_; block = pol_code(kPolUb, i, t); }
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
          if (a_ < alpha) { alpha = a_; block = pol_code(kPolSess, i, ks); }
        }
      }
      for (int k = tid; k < nrow * Tm; k += kPolThreads) {
        const int r = k / Tm, t = k - r * Tm, j = row_j(r);
        if ((RACT[r] >> t) & 1u) continue;
        const double lim = r < M ? A.limits[r] : A.peak[(size_t)b * Tm + t];
        if (!(lim < 1e299)) continue;
        if (row_is_disc(r)) {
          const double u0 = U[j * Tm + t], u1 = U[(j + M) * Tm + t], d0 = DU[j * Tm + t], d1 = DU[(j + M) * Tm + t];
          const double aa = d0 * d0 + d1 * d1, bb = 2.0 * (u0 * d0 + u1 * d1), cc = u0 * u0 + u1 * u1 - lim * lim;
          if (aa > 1e-28 && (bb > 0 || cc > 0)) {
            const double dsc = bb * bb - 4.0 * aa * cc;
            if (dsc >= 0) {
              const double a_ = fmax((-bb + sqrt(dsc)) / (2.0 * aa), 0.0);
              if (a_ < alpha) { alpha = a_; block = pol_code(kPolRow, r, t); }
            }
          }
        } else {
          const double du = DU[j * Tm + t];
          if (du > 1e-14) {
            const double a_ = fmax((lim - U[j * Tm + t]) / du, 0.0);
            if (a_ < alpha) { alpha = a_; block = pol_code(kPolRow, r, t); }
          }
        }
      }
      pol_block_argmin(alpha, block, RED);
      if (block < 0) alpha = 1.0;
      POL_TICK(5);
      // ---- (9) move; the new multipliers; the blocking constraint joins the working set ------------------------------------------------
      double xm = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) { xv[k] += alpha * dv[k]; xm = fmax(xm, fabs(xv[k])); }
      const double step = pol_block_max(stepl, RED);
      const double xmax = pol_block_max(xm, RED);
      for (int k = tid; k < nrow * Tm; k += kPolThreads) NU[k] = 0.0;
      __syncthreads();
      for (int a = tid; a < m; a += kPolThreads)
        if (RR[a] >= 0) NU[RR[a] * Tm + RT[a]] = LAM[a];
      if (block >= 0) {
        const int kind = block >> 24, p0 = (block >> 8) & 0xffff, p1 = block & 0xff;
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
          RACT[p0] |= 1u << p1;
        }
      }
      __syncthreads();
      // noise floor (oracle/polish_ref.py): full steps that have stopped shrinking go to the multiplier test and the KKT check
      // like a converged one; the check decides, and a failure there ends the polish instead of burning the round limit
      if (block < 0) {
        stall = step >= 0.5 * best_step ? stall + 1 : 0;
        best_step = fmin(best_step, step);
      } else {
        stall = 0; best_step = 1e300;
      }
      const bool floor_hit = block < 0 && stall >= kPolStallRounds && step <= 1e-3;
      const bool conv = block < 0 && (step <= kPolTolStep * fmax(1.0, xmax) || floor_hit);
      POL_TICK(6);
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
        if (((atlb >> k) & 1u) && gr < worst) { worst = gr; who = pol_code(kPolLb, i, t); }
        if (((atub >> k) & 1u) && -gr < worst) { worst = -gr; who = pol_code(kPolUb, i, t); }
      }
      if (!eq && h == 0) {
#pragma unroll
        for (int ks = 0; ks < kMaxK; ++ks)
          if (sact[ks] && smu[ks] < worst) { worst = smu[ks]; who = pol_code(kPolSess, i, ks); }
      }
      for (int k = tid; k < nrow * Tm; k += kPolThreads) {
        const int r = k / Tm, t = k - r * Tm;
        if (((RACT[r] >> t) & 1u) && NU[k] < worst) { worst = NU[k]; who = pol_code(kPolRow, r, t); }
      }
      pol_block_argmin(worst, who, RED);
      if (who >= 0) {
        const int kind = who >> 24, p0 = (who >> 8) & 0xffff, p1 = who & 0xff;
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
          RACT[p0] &= ~(1u << p1);
          NU[p0 * Tm + p1] = 0.0;
        }
        stall = 0; best_step = 1e300;
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
      for (int k = tid; k < Mg * Tm; k += kPolThreads) {
        const int j = k / Tm, t = k - j * Tm;
        double s = 0;
        for (int e = 0; e < N; ++e) s += Gs[j * N + e] * Xs[e * Tm + t];
        U[k] = s;
      }
      __syncthreads();
      for (int k = tid; k < nrow * Tm; k += kPolThreads) {
        const int r = k / Tm, t = k - r * Tm, j = row_j(r);
        const double lim = r < M ? A.limits[r] : A.peak[(size_t)b * Tm + t];
        if (!(lim < 1e299)) continue;
        const double val = row_is_disc(r) ? hypot(U[j * Tm + t], U[(j + M) * Tm + t]) : U[j * Tm + t];
        pvl = fmax(pvl, (val - lim) / fmax(1.0, lim));
      }
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
          const int j = row_j(r);
          if (row_is_disc(r)) {
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
    POL_TICK(7);
    if (tid == 0) {
      for (int ph = 0; ph < 8; ++ph) atomicAdd(A.stats + 8 + ph, (int)tacc[ph]);
      atomicAdd(A.stats + 6, rounds);
    }
#undef POL_TICK
    if (success) {
      double ol = 0;
#pragma unroll
      for (int k = 0; k < kPolTQ; ++k) {
        const int t = h * TQ + k;
        if (iv && k < TQ && t < Tm) {
          A.x[((size_t)b * N + i) * Tm + t] = xv[k];
          ol += (0.5 * pd_user * xv[k] + qv[k]) * xv[k];
        }
      }
      const double o = pol_block_sum(ol, RED);
      // site-row multipliers in the caller's units (a disc's pair: nu times its outward normal, at the final x: U is current)
      for (int k = tid; k < Mg * Tm; k += kPolThreads) A.y[(size_t)b * Mg * Tm + k] = 0.0;
      __syncthreads();
      for (int k = tid; k < nrow * Tm; k += kPolThreads) {
        const int r = k / Tm, t = k - r * Tm, j = row_j(r);
        const double nu = NU[k];
        if (nu == 0.0) continue;
        if (row_is_disc(r)) {
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
}

}  // namespace acnqp
