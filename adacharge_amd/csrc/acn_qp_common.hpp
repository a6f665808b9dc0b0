// What every kernel of the batched MPC QP solver shares: the argument block, row-type and status constants, the
// work queue, the MFMA operand map, the cross-lane primitives, the fast reciprocals and the solver's constants and
// status rules.  (The rules of the residual check itself are in acn_qp_check.hpp.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acn_qp_check.hpp"

namespace acnqp {

#ifdef ACNQP_STAMPS
// diagnostic build only: cycles per phase, [block][wave][8]; never read by the kernel
__device__ unsigned long long g_stamps[1024 * 16 * 12];
#define STAMP(slot)                                                                    \
  do {                                                                                 \
    unsigned long long _t;                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory");         \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    st_acc[slot] += _t - st_prev;                                                      \
    st_prev = _t;                                                                      \
  } while (0)
#else
#define STAMP(slot) do {} while (0)
#endif

#ifndef ACNQP_GUARD_MAX
#define ACNQP_GUARD_MAX 120   // safety bound on water-filling passes per session and iteration
#endif

constexpr int kMaxK = 4;       // session slots per EVSE
struct TiledArgs {
  int B, N, Tm, K, NP, MR;     // NP = 16 * waves (padded EVSEs), MR = 16 * MT (padded site rows)
  const void *G, *Ghat, *Q, *lam, *rowlim;   // [MR][NP], [MR][NP], [MR][MR], [MR], [MR]  (real)
  const int32_t* rowtype;                     // [MR]
  const void *fragG, *fragQ;                  // Ghat, Q as MFMA A-operand fragments: [NW][MT][2][4][64], [MT][MT][2][4][64]
  const void *fragG2, *fragQ2;                // the same blocks with the k-slices as two pairs per lane: [..][2][64][2] (acn_qp_long.hpp)
  const int32_t* horizon;
  const int32_t* order;                       // [B] or null: queue position -> problem (longest expected first, acn_qp_api.hip)
  int32_t* queue;                             // launch counter (zeroed on the stream before the launch): the grid is the chip's
                                              // resident workgroup slots and every workgroup fetches its next queue position
                                              // with one atomicAdd until the B problems are gone (null: workgroup w solves
                                              // position w -- ACNQP_NO_QUEUE=1, the static schedule)
  const double *lb, *ub, *q, *pdiag;
  const int32_t *s_off, *s_len;
  const double* s_cap;
  const uint8_t* s_eq;
  const double* peak;
  const double* lf;
  const double *dc, *dfloor;
  const double *warm_x, *warm_y;   // optional warm start (both or neither): a schedule [B][N][Tm] and site-row multipliers
                                   // [B][Mg][Tm] in the row order and units of acnqp_site.G
  const int32_t* rowabi;           // [MR] internal row -> row of acnqp_site.G (-1: padding)
  const void* rowscale;            // [MR] (real) equilibration factor of the internal row: y_abi = scale * y_internal
  int Mg;                          // rows of acnqp_site.G
  double* x;
  double* y_out;                   // optional: the site-row multipliers at exit, [B][Mg][Tm]
  int32_t *status, *iters;
  double *pri, *dua, *obj;
  double eps_abs, eps_rel, rho0, sigma, alpha, adapt_tol, reg_rel;
  double peak_scale, flat_scale, max_scale;   // host-side row equilibration of the prox rows
  int max_iter, check_every, adapt_every;
  int accel_mem;   // Anderson-acceleration columns actually used (<= the kernel's AM, fits its LDS); 0 = off
  // acnqp_options.stall_iters / inaccurate_floor / retry_* (include/acn_qp.h)
  int stall_iters, retry_passes, retry_max_iter;
  double inacc_floor, retry_rho;
  int pbuf_single; // 1: one partial-tile slab instead of two (one more barrier per iteration, LDS for one more ring column)
  // -- the polish (acn_qp_polish.hpp): a pass-0 problem that has not converged after polish_iters iterations (0 = off) leaves
  //    the solver kernel with the internal status kStatusPolish, its iterate in x / y_out, and its index appended to pol_list;
  //    `resume` = 1 is the launch that follows the polish kernel: it runs over pol_list (order = pol_list, count_dev = its
  //    length, on the device), skips what the polish solved and solves the rest from scratch as if there were no polish
  int polish_iters, resume;
  int polish_stall;           // > 0: from polish_iters / 2 on, a problem whose residual score has not improved by 10 % for this many
                              // iterations is handed over early (acn_qp_wave.hpp; acn_qp_api.hip sets polish_iters / 4)
  int y_for_polish_only;      // 1: y_out is the polish's internal buffer -- only a problem that is handed over writes it (the
                              // multipliers of every problem were 5.4 KB of HBM writes per problem for 1.5 KB of payload)
  int pol_rows;               // rows of the polish kernel's Schur system for this shape: a problem whose iterate has more tight site
                              // rows than that is not handed over (it would come straight back) and the ADMM goes on
  int32_t *pol_list, *pol_count;
  int32_t* pol_retired;       // null, or (wave kernel, work-queue launches): the problems of this launch that are finished and, where
                              // handed over, published -- what a polish launch running ALONGSIDE this one waits for
  const int32_t* count_dev;   // number of queue positions, on the device (null: B)
  double* const* x_host;      // null, or (wave kernel, one wave per problem: Route::direct_x) [B] device-addressable HOST destinations
                              // of the problems' schedules (null entry: none): the wave that gives problem b its verdict also
                              // stores x there, in flat order -- the host entries then copy no x back
  const double* const* lb_host;   // null, or (wave kernel, one wave per problem: Route::direct_in) [B] device-addressable HOST sources of
  const double* const* ub_host;   // the problems' lb / ub / q (the three entries of a problem are set together; null entries: read the
  const double* const* q_host;    // device copy as ever): the wave that starts problem b in pass 0 loads them from there in flat order
                                  // and stores them into lb / ub / q, which the host entry then has not copied
  int ws_by_slot;  // 1: a streaming kernel's workspace belongs to the workgroup slot (work-queue launches), 0: to the problem
  int grid_oversub; // host side only: workgroups of a work-queue launch per resident slot (1: fully persistent; the pipelined
                    // host entries use 4, so that slots come free while a launch runs and the next stream's small launches --
                    // the polish, the resume -- do not wait for a whole persistent launch to drain)
  int grid_cap;    // host side only: most workgroups a launch may have (the kernels that stream their state own one
                   // workspace per workgroup slot)
};

typedef const __attribute__((address_space(4))) TiledArgs* KernargPtr;   // the kernel's own argument block

// ---- work queue (all four kernel families) ----------------------------------------------------------------------------
// A launch of B problems on S resident workgroup slots used to be B workgroups handed out in index order: a slot's
// share of the work was whatever its problems happened to need, and the launch ended with its slowest slot (configs[4]
// leg, 2,048 problems on 512 slots: the last slot at ~2,200 iterations, the mean slot at 1,525).  Now the grid is the S
// slots and a workgroup that finishes a problem takes the next queue position: one atomicAdd by thread 0, broadcast
// through LDS.  Returns the position (block-uniform, a scalar), or -1 when the launch has no problem left for this
// workgroup.  `round` counts this workgroup's fetches (the static fallback serves exactly one).  Both barriers are
// needed: the first publishes the slot, the second keeps a fast wave's next fetch from overwriting it before a slow wave
// has read it -- and orders the previous problem's last LDS reads before the next problem's first LDS writes.
__device__ inline int queue_length(const TiledArgs& a) {
  if (a.count_dev == nullptr) return a.B;
  const int n = *a.count_dev;
  return n < a.B ? n : a.B;
}
__device__ inline int queue_next(int32_t* queue, int B, int round, int* slot_lds) {
  if (queue == nullptr) return round == 0 && (int)blockIdx.x < B ? (int)blockIdx.x : -1;
  if (threadIdx.x == 0) *slot_lds = atomicAdd(queue, 1);
  __syncthreads();
  const int pos = __builtin_amdgcn_readfirstlane(*slot_lds);
  __syncthreads();
  return pos < B ? pos : -1;
}

template <typename real> struct Mfma;
template <> struct Mfma<double> {
  typedef double vec4 __attribute__((ext_vector_type(4)));
  __host__ __device__ static constexpr int rowof(int g, int r) { return g + 4 * r; }
  __device__ static inline vec4 mma(double a, double b, vec4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static constexpr double proj_tol = 1e-13;
  static constexpr double big = 1e300;
};

// ---- cross-lane helpers (DPP: plain VALU moves, no LDS crossbar) -------------------------------
template <int CTRL> __device__ inline float dpp_mov(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int CTRL> __device__ inline double dpp_mov(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kRowHalfMirror = 0x141, kRowMirror = 0x140;

// reductions over the 16 lanes of a DPP row (= the 16 periods of one EVSE); every lane gets the result
template <typename T> __device__ inline T row_sum(T v) {
  v += dpp_mov<kQuadXor1>(v);
  v += dpp_mov<kQuadXor2>(v);
  v += dpp_mov<kRowHalfMirror>(v);
  v += dpp_mov<kRowMirror>(v);
  return v;
}
template <typename T> __device__ inline T row_min(T v) {
  v = fmin(v, dpp_mov<kQuadXor1>(v));
  v = fmin(v, dpp_mov<kQuadXor2>(v));
  v = fmin(v, dpp_mov<kRowHalfMirror>(v));
  v = fmin(v, dpp_mov<kRowMirror>(v));
  return v;
}
template <typename T> __device__ inline T row_max(T v) {
  v = fmax(v, dpp_mov<kQuadXor1>(v));
  v = fmax(v, dpp_mov<kQuadXor2>(v));
  v = fmax(v, dpp_mov<kRowHalfMirror>(v));
  v = fmax(v, dpp_mov<kRowMirror>(v));
  return v;
}

// A block-uniform double moved to the scalar unit (two v_readfirstlane): it then occupies a scalar register pair instead of
// two vector registers per lane for as long as it lives (the kernels' penalty, its reciprocals, norms, scores ...).
__device__ inline double uniform_scalar(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// A double constant materialised in a scalar register pair where it is used (two s_mov_b32), opaque to the optimiser:
// without this the compiler hoists every such constant of the kernel (1e300, 1.2, 0.9, 1e-300, 1e-6 ...) into a vector
// register pair at the top and keeps -- or spills -- it across the solver loop.
__device__ inline double scalar_const(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
  asm volatile("" : "+s"(lo), "+s"(hi));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// The value lane `src` holds (src uniform), as a scalar: v_readlane instead of the LDS crossbar a __shfl goes through
__device__ inline double lane_value(double v, int src) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, src), hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
struct ScalarConst { __device__ static inline double c(double v) { return scalar_const(v); } };   // acn_qp_check.hpp's literals, that way
__device__ inline float uniform_scalar(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, v))); }

// 1 / sqrt(x): hardware estimate + two Newton steps (full precision for f64, cheaper than sqrt + div)
__device__ inline double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - 0.5 * x * y * y);
  y = y * (1.5 - 0.5 * x * y * y);
  return y;
}
__device__ inline float rsqrt_nr(float x) {
  float y = __builtin_amdgcn_rsqf(x);
  y = y * (1.5f - 0.5f * x * y * y);
  return y;
}

// 1 / x for x > 0: hardware estimate + Newton steps (avoids the long IEEE division sequence)
__device__ inline double rcp_nr(double x) {
  double y = __builtin_amdgcn_rcp(x);
  y = y + y * (1.0 - x * y);
  y = y + y * (1.0 - x * y);
  return y;
}
__device__ inline float rcp_nr(float x) {
  float y = __builtin_amdgcn_rcpf(x);
  y = y + y * (1.0f - x * y);
  return y;
}

// 1 / n for a small positive integer n (interior-period count of a session window)
__device__ inline double rcp_small(float nf) {
  const double x = (double)nf;
  double y = (double)__builtin_amdgcn_rcpf(nf);   // ~1e-7 relative
  y = y + y * (1.0 - x * y);                      // ~1e-14
  y = y + y * (1.0 - x * y);                      // full double precision
  return y;
}

// Anderson acceleration of the ADMM fixed-point map (restated in oracle/admm_port.c, see there)
constexpr double kStartGain = 1e5;   // (adacharge_amd/rollout.py START_GAIN restates it: a warm start's arriving sessions)
// Tikhonov floor (options.reg_rel) -- applied ONLY to problems whose own objective cannot select a unique point:
// no prox row in use (load_flattening / demand_charge weights zero) and a quadratic the solver cannot resolve,
// pdiag * max(ub) <= kRegResolve * |q|_inf (pure LPs; the reference's equal_share * 1e-12).  A strictly convex
// problem is solved exactly as stated (the reference passes no solver options, aco.py:315-321).
constexpr double kRegResolve = 1e-6;
template <typename real>
__host__ __device__ inline real effective_pdiag(real pd_user, real reg_rel, real qnorm, real ubmax, int horizon, bool has_prox) {
  if (has_prox || !(ubmax > (real)0) || pd_user * ubmax > (real)kRegResolve * qnorm) return pd_user;
  const real fl = reg_rel * qnorm / (ubmax * (real)(horizon > 1 ? horizon : 1));
  return fl > pd_user ? fl : pd_user;
}
// SOLVED_INACCURATE (the reference accepts cvxpy's OPTIMAL_INACCURATE, aco.py:319): when the iteration limit or the
// stall rule ends a problem with both residuals within kInaccurate x the requested tolerance, or within the tolerance
// cvxpy hands OSQP by default (eps_abs = eps_rel = 1e-5), whichever is looser.
constexpr double kInaccurate = 100.0;
template <typename real>
__host__ __device__ inline bool inaccurate_ok(real pri, real dua, real npri, real ndua, double eps_abs, double eps_rel, double floor_) {
  const real ea = (real)(kInaccurate * eps_abs > floor_ ? kInaccurate * eps_abs : floor_);
  const real er = (real)(kInaccurate * eps_rel > floor_ ? kInaccurate * eps_rel : floor_);
  return pri <= ea + er * npri && dua <= ea + er * ndua;
}
// Retry passes (acnqp_options.retry_passes): a problem that ends a pass MAX_ITER / SOLVED_INACCURATE after at least
// retry_min_iters(stall_iters) iterations is solved again, inside the same kernel, from a cold start with a FIXED
// penalty retry_rho * 4^(pass - 1) (no adaptation) and at most retry_max_iter iterations.  Why: traced on the C twin
// (DESIGN.md section 2), the congested instances that sit on a plateau of the primal residual do so because the penalty
// adaptation swings rho by 10x several times in the first few hundred iterations and the iterate ends in a region it
// leaves only sub-linearly; from a cold start with a fixed rho in [0.3, 4] every one of them converges in 900 ... 4,400
// iterations -- while a fixed rho for everybody would double the iterations of the average problem.  The answer of
// the best pass is the one returned (SOLVED beats SOLVED_INACCURATE beats MAX_ITER; the first of equals), iters is
// the total over the passes.
__host__ __device__ inline int retry_min_iters(int stall_iters) { return stall_iters > 0 ? stall_iters : 3000; }
__host__ __device__ inline int status_rank(int st) { return st == 1 ? 3 : (st == 5 ? 2 : (st == 2 ? 1 : 0)); }
__host__ __device__ inline bool retry_wanted(int pass, int retry_passes, int status, int it, int stall_iters, int adapt_every0) {
  return pass < retry_passes && (status == 2 || status == 5) && it >= retry_min_iters(stall_iters) && adapt_every0 > 0;
}
constexpr int kAaPeriod = 5;
constexpr double kAaReg = 1e-4, kAaSafe = 1.2, kAaDrift = 1e-3;

// Reductions over the lanes l, l^16, l^32, l^48 (the four quarter-lanes of one EVSE in session
// layout) with v_permlane16_swap / v_permlane32_swap: swapping a register with itself leaves the
// two partner values in the two results for EVERY lane, so r[0] (op) r[1] is the pairwise result --
// plain VALU, no LDS crossbar, and bitwise identical in both partners.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
struct Pair32 { unsigned a, b; };
struct PairF { float a, b; };
struct PairD { double a, b; };
template <int WHICH> __device__ inline Pair32 swap_u32(unsigned v) {
  const u32x2 r = WHICH == 16 ? __builtin_amdgcn_permlane16_swap(v, v, false, false)
                              : __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return {r[0], r[1]};
}
template <int WHICH> __device__ inline PairF swap_pair(float v) {
  const Pair32 p = swap_u32<WHICH>(__builtin_bit_cast(unsigned, v));
  return {__builtin_bit_cast(float, p.a), __builtin_bit_cast(float, p.b)};
}
template <int WHICH> __device__ inline PairD swap_pair(double v) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
  const Pair32 lo = swap_u32<WHICH>((unsigned)(bits & 0xffffffffull));
  const Pair32 hi = swap_u32<WHICH>((unsigned)(bits >> 32));
  return {__builtin_bit_cast(double, ((unsigned long long)hi.a << 32) | lo.a),
          __builtin_bit_cast(double, ((unsigned long long)hi.b << 32) | lo.b)};
}
template <typename T> __device__ inline T quarter_sum(T v) {
  auto p = swap_pair<16>(v); v = p.a + p.b;
  auto q = swap_pair<32>(v); return q.a + q.b;
}
template <typename T> __device__ inline T quarter_min(T v) {
  auto p = swap_pair<16>(v); v = fmin(p.a, p.b);
  auto q = swap_pair<32>(v); return fmin(q.a, q.b);
}
template <typename T> __device__ inline T quarter_max(T v) {
  auto p = swap_pair<16>(v); v = fmax(p.a, p.b);
  auto q = swap_pair<32>(v); return fmax(q.a, q.b);
}

template <typename T> __device__ inline T wave_max(T v) { return quarter_max<T>(row_max<T>(v)); }
template <typename T> __device__ inline T wave_sum(T v) { return quarter_sum<T>(row_sum<T>(v)); }

}  // namespace acnqp
