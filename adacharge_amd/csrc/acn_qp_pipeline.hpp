// The host-buffer entries' pipeline (acnqp_solve_batches, acnqp_solve_table): a call is cut into chunks that rotate
// over the handle's kSlots streams, so that the H2D copies, the kernels and the D2H copies of successive chunks overlap.
// ONE planner, ONE chunk loop and ONE epilogue for both entries; they differ in how a chunk's inputs reach the device
// (fill_dense / fill_table) and in nothing else.
//
// Part 1 (chunk layout and planner) is plain host code: tests/test_route_table.py compiles it with the host compiler.
// Part 2 (the kernels of this unit, the chunk loop) belongs to the API translation unit: acn_qp_api.hip includes this
// file after acnqp_handle, fail() and HIP_TRY.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace acnqp {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// device layout of one chunk of `cn` problems (inputs in slot.in, results in slot.out)
struct ChunkLayout {
  size_t lb, ub, q, pd, hz, so, sl, sc, eq, pk, lf, dc, df, xh, wx, wy, in_total;
  size_t x, st, it, pr, du, ob, y, out_total;
  // direct: the chunk carries the host destinations of its problems' schedules (xh: one double* per problem, a small input)
  ChunkLayout(size_t cn, size_t N, size_t Tm, size_t K, size_t Mg, bool peak, bool flat, bool mx, bool warm, bool want_y, bool direct = false) {
    size_t o = 0;
    lb = o; o += al256(cn * N * Tm * 8);
    ub = o; o += al256(cn * N * Tm * 8);
    q = o;  o += al256(cn * N * Tm * 8);
    pd = o; o += al256(cn * 8);
    hz = o; o += al256(cn * 4);
    so = o; o += al256(cn * K * N * 4);
    sl = o; o += al256(cn * K * N * 4);
    sc = o; o += al256(cn * K * N * 8);
    eq = o; o += al256(cn);
    pk = o; o += al256(peak ? cn * Tm * 8 : 0);
    lf = o; o += al256(flat ? cn * 8 : 0);
    dc = o; o += al256(mx ? cn * 8 : 0);
    df = o; o += al256(mx ? cn * 8 : 0);
    xh = o; o += al256(direct ? cn * sizeof(double*) : 0);
    wx = o; o += al256(warm ? cn * N * Tm * 8 : 0);
    wy = o; o += al256(warm ? cn * Mg * Tm * 8 : 0);
    in_total = o;
    o = 0;
    x = o;  o += al256(cn * N * Tm * 8);
    st = o; o += al256(cn * 4);
    it = o; o += al256(cn * 4);
    pr = o; o += al256(cn * 8);
    du = o; o += al256(cn * 8);
    ob = o; o += al256(cn * 8);
    y = o;  o += al256(want_y ? cn * Mg * Tm * 8 : 0);
    out_total = o;
  }
};

// ---- the planner ----------------------------------------------------------------------------------------------------------
// diagnostic variables of the planner, read at every call (acn_qp_api.hip)
struct PlanEnv {
  long long chunk = 0;          // ACNQP_CHUNK > 0: problems per chunk instead of the route's wanted size
  const char* plan = nullptr;   // ACNQP_PLAN "a,b,c": explicit chunk sizes of a planned (wave) call; the rest goes into a last chunk
  bool ramp = true;             // ACNQP_NO_RAMP unset
  bool direct = false;          // not a variable: the kernel stores every schedule of the call into the caller's host arrays
                                // (Route::direct_x, run_call), so no copy of x stands behind the last launch
};

// inputs + results staged per problem -- every one of the kSlots pipeline slots holds a chunk of each, so a chunk is
// capped at 1 GiB of the sum.  (The kernels' workspaces belong to the resident workgroup slots: no per-problem term.)
inline long long chunk_cap_by_memory(size_t N, size_t Tm, size_t K) {
  const size_t per_problem = 4 * N * Tm * 8 + K * N * 16 + Tm * 8 + 96;
  return (long long)((size_t)1024 * 1024 * 1024 / std::max<size_t>(per_problem, 1));
}

// The chunk caps of a call of `total` problems: chunk c takes up to chunk_cap(caps, c) problems.  `want`: what the route
// asks for (Route::chunk_want); `wave`: the wave kernel serves the shape; `uniform`: the whole call has one shape and
// one set of optional arrays (the session-table entry always).
//  * A uniform wave call is planned as a whole: a quarter-size and a half-size chunk in front (the first kernel waits
//    for its inputs, and nothing overlaps that copy), full chunks, and a quarter-size one at the END (what follows the
//    last solver launch -- its polish, its result copies -- is exposed too): c/4 + c/2 + k c + c/4 = total with the
//    smallest k for which c <= cap.  Fewer than 2,048 problems (or a cap below that) make one chunk.
//  * ... with env.direct (the kernel writes the schedules to the caller's arrays itself) without the small last chunk:
//    u, 2u, 2u in front, then chunks of 3u (below).
//  * Every other call ramps: a quarter-size first chunk, then a half-size one, then full ones.
inline std::vector<long long> plan_chunk_caps(long long total, long long want, long long by_mem, bool wave, bool uniform,
                                              const PlanEnv& env) {
  if (env.chunk > 0) want = env.chunk;
  long long cap = std::max<long long>(1, std::min(want, by_mem));
  if (cap >= 512) cap -= cap % 512;   // whole rounds of the chip's 512 workgroup slots (2 per CU): no thin last round
  std::vector<long long> caps;
  if (env.ramp && wave && uniform) {
    if (env.plan) {
      // (an entry below 1 would never end the call: clamped)
      for (const char* q = env.plan; *q;) { caps.push_back(std::max<long long>(1, std::atoll(q))); while (*q && *q != ',') ++q; if (*q == ',') ++q; }
    } else if (env.direct && total >= 2048 && cap >= 2048) {
      // Nothing but the copy of the small result arrays follows the last launch, so the small last chunk goes: in units of
      // u the chunks are u, 2u, 2u in front and then m chunks of 3u -- 2,048 / 4,096 / 4,096 / 6,144 for 16,384 problems --
      // with u = ceil(total / (5 + 3 m)) and the smallest m >= 1 for which 3u <= cap; the front takes what the m last
      // chunks leave (f <= 5u problems: f/5, 2f/5 and the rest).  The last chunk is the largest: its launch starts when
      // its inputs have landed, and the inputs of the whole call land only two thirds into the step (41 GB/s measured
      // on the headline step), so what it holds is what the chip has left to do from then on; a last chunk of half the call
      // (u, u, 2u, 4u) measured no gain over the copy path, the small one of the copy path's plan 0.15 ms.
      long long m = 1, u = 0;
      for (;; ++m) {
        u = (total + 4 + 3 * m) / (5 + 3 * m);
        if (3 * u <= cap) break;
      }
      const long long f = total - 3 * u * m;   // (> 0: with m - 1 last chunks 3u was above the cap, so total > (2 + 3m) u)
      caps.push_back(std::max<long long>(1, f / 5));
      caps.push_back(std::max<long long>(1, 2 * f / 5));
      caps.push_back(std::max<long long>(1, f - f / 5 - 2 * f / 5));
      for (long long i = 0; i < m; ++i) caps.push_back(3 * u);
    } else if (total >= 2048 && cap >= 2048) {
      const long long k = (total + cap - 1) / cap - 1;
      long long c = total / (k + 1);
      c = std::max<long long>(2048, std::min(cap, c - c % 512));
      caps.push_back(c / 4);
      caps.push_back(c / 2);
      for (long long i = 0; i < k; ++i) caps.push_back(c);
    }
    caps.push_back(std::max<long long>(1, total));   // the rest
  } else if (env.ramp && cap >= 1024) {
    caps = {cap / 4, cap / 2, cap};
  } else {
    caps = {cap};
  }
  return caps;
}
inline long long chunk_cap(const std::vector<long long>& caps, size_t c) { return caps[std::min(c, caps.size() - 1)]; }

}  // namespace acnqp

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

#include "acn_qp.h"
#include "acn_qp_route.hpp"

namespace {

using acnqp::al256;
using acnqp::ChunkLayout;

// ---- launch order: longest expected problem first -------------------------------------------------------------------
// A launch of B problems on S resident workgroup slots ends with its slowest slot; the hardware hands workgroups out in
// index order, so the tail is up to one whole problem long (bench workload, 32 problems per slot: natural order 7.0 %
// above the mean slot, `longest first` by the TRUE iteration counts 0.2 %).  Two tiny kernels give every problem a key
// that predicts its iteration count and sort the problems by it, descending; every solver kernel maps workgroup ->
// problem through the result.  Results do not depend on the order (a workgroup only touches its own problem).
//
// Which key.  Measures of DEMAND (sessions, sum of s_len, sum of ub, deliverable energy) do not level the wave kernel's
// headline launch (16 problems per slot on 1,024 wave slots): a handful of problems with few sessions run 400 ... 808
// iterations, start late under such a key and end late.  What sets the iteration count is CONGESTION: how much of the
// schedule that ignores the site rows the site rows reject.  The key is computed from the GREEDY schedule x0 (every
// session charges at its upper bound from its first period until its energy cap is used up): C = the (site row, period)
// cells whose load under x0 exceeds the limit, key = 8 min(C, 127) + min(7, sessions / 8).  A problem with C = 0
// converges at the first residual check (20 iterations; exactly so on the 49,152 problems of three bench seed sets, 36 %
// of them), so every queue ends with fine-grained work.  tests/order_key_spec.py is the definition in numpy,
// tools/sim_launch_tail.py the SIMULATION that chose the key on the CPU twin's iteration counts (wave-iterations, mean of
// three seed sets, lone launch / chunk plan: even spread 3,113; sessions 3,656 / 3,936; this key 3,436 / 3,816; the
// true iteration counts 3,120 / 3,515; profiles/order_key_sim.json), DESIGN.md section 3.7 what it measured.
// ACNQP_ORDER_KEY=sessions / overload (diagnostic, read once per process) selects the key in the same binary.
constexpr int kOrderKeys = 1024;
constexpr int kOrderMinBatch = 768;   // fewer problems than ~1.5 x the resident slots: nothing to level
// LDS budget of order_keys_kernel: the greedy schedule of ONE problem (N x Tm doubles) may take 64 KB (54 x 144 fits), and
// a workgroup -- the site's infrastructure rows of G, then the schedules of its waves -- the CU's 160 KB.  A shape beyond
// either gets the session-count key; a shape whose four schedules do not fit one workgroup gets fewer waves per workgroup.
// Decided by shape (order_key_waves), never by batch.
constexpr size_t kOrderLdsPerProblem = (size_t)64 << 10;
constexpr size_t kOrderLdsPerGroup = (size_t)160 << 10;
inline int order_key_waves(size_t N, size_t Tm, size_t g_rows) {   // waves (= problems) per workgroup; 0: session-count key
  const size_t sched = N * Tm * sizeof(double), g = g_rows * N * sizeof(double);
  if (sched == 0 || sched > kOrderLdsPerProblem || g + sched > kOrderLdsPerGroup) return 0;
  return (int)std::min<size_t>(4, (kOrderLdsPerGroup - g) / sched);
}

// the session-count key: ACNQP_ORDER_KEY=sessions, and every shape beyond the LDS budget of order_keys_kernel
__global__ __launch_bounds__(256) void session_keys_kernel(const int32_t* s_len, int KN, int B, int32_t* keys) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;
  int c = 0;
  for (int k = lane; k < KN; k += 64) c += s_len[(size_t)b * KN + k] > 0 ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) keys[b] = c < kOrderKeys ? c : kOrderKeys - 1;
}

struct OrderKeyArgs {
  int B, N, Tm, K, M, soc, has_peak;   // M infrastructure constraints: G rows [0, M) and, for SOC, their partners [M, 2M)
  const double *lb, *ub, *s_cap, *peak, *G, *limits;   // G, limits: acnqp_site's, in the caller's row order and units
  const int32_t *s_off, *s_len, *horizon;
  int32_t* keys;
};

// The congestion key (above; tests/order_key_spec.py).  One wave per problem, blockDim.x / 64 problems per workgroup.
// LDS: the infrastructure rows of G (staged once per workgroup), then one schedule x0[N][Tm] per wave.  Phase 1, a lane
// per (session slot, EVSE): the greedy schedule over the slot's window (windows of one EVSE are disjoint: no two lanes
// write one entry).  Phase 2, a lane per (row, period) cell: the row's load under x0 against its limit.
__global__ __launch_bounds__(256) void order_keys_kernel(const OrderKeyArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char order_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int N = a.N, Tm = a.Tm, M = a.M;
  const int g_rows = a.soc ? 2 * M : M;
  double* Gs = reinterpret_cast<double*>(order_lds);
  double* x0 = Gs + (size_t)g_rows * N + (size_t)wave * N * Tm;
  const int b = blockIdx.x * (int)(blockDim.x >> 6) + wave;
  const bool live = b < a.B;   // (a wave without a problem still takes part in the barriers)
  for (int k = threadIdx.x; k < g_rows * N; k += blockDim.x) Gs[k] = a.G[k];
  if (live)
    for (int k = lane; k < N * Tm; k += 64) x0[k] = 0.0;
  __syncthreads();
  int sessions = 0;
  if (live) {
    const int hz = min(a.horizon[b], Tm);
    const size_t sb = (size_t)b * a.K * N, vb = (size_t)b * N * Tm;
    for (int k = lane; k < a.K * N; k += 64) {
      const int len = a.s_len[sb + k];
      if (len <= 0) continue;
      ++sessions;
      const int i = k % N, off = a.s_off[sb + k];
      const int t0 = max(off, 0), t1 = (int)min((long long)off + len, (long long)hz);   // (inside [0, Tm) whatever the arrays hold)
      double rem = a.s_cap[sb + k];
      for (int t = t0; t < t1; ++t) {
        const double d = fmax(a.lb[vb + (size_t)i * Tm + t], fmin(a.ub[vb + (size_t)i * Tm + t], fmax(rem, 0.0)));
        x0[i * Tm + t] = d;
        rem -= d;
      }
    }
  }
  __syncthreads();
  int over = 0;
  if (live) {
    const int cells = (M + (a.has_peak && a.peak ? 1 : 0)) * Tm;
    for (int c = lane; c < cells; c += 64) {
      const int j = c / Tm, t = c - j * Tm;
      double load, limit;
      if (j < M) {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < N; ++i) re += Gs[j * N + i] * x0[i * Tm + t];
        if (a.soc)
          for (int i = 0; i < N; ++i) im += Gs[(j + M) * N + i] * x0[i * Tm + t];
        load = a.soc ? hypot(re, im) : re;
        limit = a.limits[j];
      } else {
        load = 0.0;
        for (int i = 0; i < N; ++i) load += x0[i * Tm + t];
        limit = a.peak[(size_t)b * Tm + t];   // (+inf: never overloaded)
      }
      // load / limit > 1 + 1e-9 without the division (no NaN of 0 / 0: this unit is compiled with -fno-honor-nans)
      over += (limit > 0.0 ? load > (1.0 + 1e-9) * limit : limit == 0.0 && load > 0.0) ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) { over += __shfl_xor(over, o); sessions += __shfl_xor(sessions, o); }
  if (live && lane == 0) a.keys[b] = min(kOrderKeys - 1, 8 * min(over, 127) + min(7, sessions / 8));
}
__global__ __launch_bounds__(kOrderKeys) void order_sort_kernel(const int32_t* keys, int B, int32_t* order) {
  __shared__ int hist[kOrderKeys], scan[kOrderKeys];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  for (int b = tid; b < B; b += kOrderKeys) atomicAdd(&hist[keys[b]], 1);
  __syncthreads();
  // slot r = kOrderKeys - 1 - key (largest key first): exclusive prefix sum over r
  scan[tid] = hist[kOrderKeys - 1 - tid];
  __syncthreads();
  for (int o = 1; o < kOrderKeys; o <<= 1) {
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  hist[kOrderKeys - 1 - tid] = scan[tid] - hist[kOrderKeys - 1 - tid];   // start of this key's run
  __syncthreads();
  for (int b = tid; b < B; b += kOrderKeys) order[atomicAdd(&hist[keys[b]], 1)] = b;
}

// ---- session-table entry: the dense problem arrays are formed on the device ---------------------------------------------
struct TableExpandArgs {
  int N, Tm, K;
  long long s_base, r_base;          // first session / rate entry of the chunk (the segment arrays hold global indices)
  const int32_t *q_index, *sess_seg, *s_evse, *s_slot, *s_off, *s_len, *rate_seg;
  const double *q_table, *s_cap, *min_rates, *max_rates;
  double *lb, *ub, *q, *sc;
  int32_t *so, *sl;
};

// One workgroup per problem of the chunk: zero its bounds and session slots, copy its horizon's linear cost, then
// scatter its sessions -- lb / ub over the window (aco.py:62-75, ub < lb -> lb) and (offset, length, cap) into the
// EVSE's slot (aco.py:105-123).  Windows of one EVSE are disjoint: no two sessions write one entry.
__global__ __launch_bounds__(256) void table_expand_kernel(const TableExpandArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t nv = (size_t)a.N * a.Tm, ns = (size_t)a.K * a.N;
  double *lb = a.lb + b * nv, *ub = a.ub + b * nv, *q = a.q + b * nv;
  const double* qt = a.q_table + (size_t)a.q_index[b] * nv;
  for (size_t k = tid; k < nv; k += 256) { lb[k] = 0.0; ub[k] = 0.0; q[k] = qt[k]; }
  for (size_t k = tid; k < ns; k += 256) { a.so[b * ns + k] = 0; a.sl[b * ns + k] = 0; a.sc[b * ns + k] = 0.0; }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const long long s0 = a.sess_seg[b] - a.s_base, s1 = a.sess_seg[b + 1] - a.s_base;
  for (long long s = s0 + wave; s < s1; s += 4) {
    const int ev = a.s_evse[s], off = a.s_off[s], len = a.s_len[s];
    const long long r0 = a.rate_seg[s] - a.r_base;
    for (int p_ = lane; p_ < len; p_ += 64) {
      const double lo = a.min_rates[r0 + p_], hi = a.max_rates[r0 + p_];
      lb[(size_t)ev * a.Tm + off + p_] = lo;
      ub[(size_t)ev * a.Tm + off + p_] = hi < lo ? lo : hi;
    }
    if (lane == 0 && len > 0) {
      const size_t k = (size_t)b * ns + (size_t)a.s_slot[s] * a.N + ev;
      a.so[k] = off; a.sl[k] = len; a.sc[k] = a.s_cap[s];
    }
  }
}

// table staging of the chunk of problems [lo, lo + cn): q_index[cn], sess_seg[cn + 1], {evse, slot, off, len}[ns],
// rate_seg[ns + 1], s_cap[ns], min / max [nr], q_table
struct TableLayout {
  long long s0 = 0, ns = 0, r0 = 0, nr = 0;
  size_t qi = 0, sg = 0, ev = 0, sl = 0, of = 0, ln = 0, rs = 0, cp = 0, mn = 0, mxr = 0, qt = 0, total = 0;
  TableLayout() = default;   // (dense entry: no table staging)
  TableLayout(const acnqp_table* T, long long lo, long long cn, size_t nv) {
    s0 = T->sess_seg[lo]; ns = T->sess_seg[lo + cn] - s0;
    r0 = T->rate_seg[s0]; nr = T->rate_seg[s0 + ns] - r0;
    size_t o = 0;
    qi = o; o += al256((size_t)cn * 4);
    sg = o; o += al256((size_t)(cn + 1) * 4);
    ev = o; o += al256((size_t)ns * 4);
    sl = o; o += al256((size_t)ns * 4);
    of = o; o += al256((size_t)ns * 4);
    ln = o; o += al256((size_t)ns * 4);
    rs = o; o += al256((size_t)(ns + 1) * 4);
    cp = o; o += al256((size_t)ns * 8);
    mn = o; o += al256((size_t)nr * 8);
    mxr = o; o += al256((size_t)nr * 8);
    qt = o; o += al256((size_t)T->n_horizons * nv * 8);
    total = o;
  }
};

// ---- a call and its chunks ---------------------------------------------------------------------------------------------
struct BatchShape { long long batch; int t_max, k_sessions; bool warm, want_y; };
struct Piece { int g; long long lo, n, pos; };   // problems [lo, lo + n) of batch g sit at [pos, pos + n) of their chunk
// what the caller's small result arrays still need after the streams have drained: a copy out of the pinned mirror
struct Scatter { int g; size_t lo, n, pos; const char* host; size_t st, it, pr, du, ob; };

// one call of a host-buffer entry: dense batches P[nb] (acnqp_solve_batches) or ONE session table T (acnqp_solve_table)
struct Call {
  const acnqp_problems* P = nullptr;
  const acnqp_table* T = nullptr;
  acnqp_results* R = nullptr;      // [nb]; the table's one
  std::vector<BatchShape> bs;
  std::vector<Scatter> scatter;    // dense entry with staged small arrays
  std::vector<double*> xdst;       // [nb] the direct path: R[g].x as the device addresses it (null: batch g keeps its copies)
};

// ---- the direct path for x ---------------------------------------------------------------------------------------------
// A result array x in device-addressable host memory (pinned: acnqp_host_alloc, hipHostMalloc, hipHostRegister) is written
// by the kernel itself where the route can do that (Route::direct_x; TiledArgs::x_host): the wave that gives a problem
// its verdict stores the schedule there, pol_x_to_host_kernel (acn_qp_api.hip) those of the handed-over problems, and the
// chunk loop queues no copy of x.  The destinations ride with the chunk's small inputs (ChunkLayout::xh), so only the
// dense entry with its pinned mirrors takes the path.  Pageable and device arrays keep their copies; a call may mix both.
// ACNQP_NO_DIRECT_X=1 (diagnostic, read once per process): the copy path everywhere.
double* direct_destination(const double* x) {
  static const bool off = std::getenv("ACNQP_NO_DIRECT_X") != nullptr;
  if (off || x == nullptr) return nullptr;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, x) != hipSuccess) {   // (memory the runtime does not know: pageable)
    (void)hipGetLastError();
    return nullptr;
  }
  return at.type == hipMemoryTypeHost ? static_cast<double*>(at.devicePointer) : nullptr;
}

// the device-side view of a chunk of cn problems laid out by L in a slot's staging (di: inputs, dq: results)
void device_views(const ChunkLayout& L, char* di, char* dq, const acnqp::SiteShape& s, size_t cn, const BatchShape& b,
                  acnqp_problems* dp, acnqp_results* dr) {
  dp->batch = (int32_t)cn; dp->t_max = b.t_max; dp->k_sessions = b.k_sessions;
  dp->lb = reinterpret_cast<const double*>(di + L.lb);
  dp->ub = reinterpret_cast<const double*>(di + L.ub);
  dp->q = reinterpret_cast<const double*>(di + L.q);
  dp->pdiag = reinterpret_cast<const double*>(di + L.pd);
  dp->horizon = reinterpret_cast<const int32_t*>(di + L.hz);
  dp->s_off = reinterpret_cast<const int32_t*>(di + L.so);
  dp->s_len = reinterpret_cast<const int32_t*>(di + L.sl);
  dp->s_cap = reinterpret_cast<const double*>(di + L.sc);
  dp->s_eq = reinterpret_cast<const uint8_t*>(di + L.eq);
  dp->peak = s.has_peak ? reinterpret_cast<const double*>(di + L.pk) : nullptr;
  dp->lf = s.has_flat ? reinterpret_cast<const double*>(di + L.lf) : nullptr;
  dp->dc = s.has_max ? reinterpret_cast<const double*>(di + L.dc) : nullptr;
  dp->dfloor = s.has_max ? reinterpret_cast<const double*>(di + L.df) : nullptr;
  dp->warm_x = b.warm ? reinterpret_cast<const double*>(di + L.wx) : nullptr;
  dp->warm_y = b.warm ? reinterpret_cast<const double*>(di + L.wy) : nullptr;
  dr->x = reinterpret_cast<double*>(dq + L.x);
  dr->status = reinterpret_cast<int32_t*>(dq + L.st);
  dr->iters = reinterpret_cast<int32_t*>(dq + L.it);
  dr->pri_res = reinterpret_cast<double*>(dq + L.pr);
  dr->dua_res = reinterpret_cast<double*>(dq + L.du);
  dr->obj = reinterpret_cast<double*>(dq + L.ob);
  dr->x_dev = nullptr;
  dr->y = b.want_y ? reinterpret_cast<double*>(dq + L.y) : nullptr;
}

// chunks: consecutive batches of one shape (t_max, k_sessions) and one set of optional arrays (warm start, multiplier
// output) share launches of up to the planner's cap
std::vector<std::vector<Piece>> split_call(const acnqp_handle* h, const std::vector<BatchShape>& bs, const acnqp::PlanEnv& env) {
  long long total = 0;
  bool uniform = true;   // one shape, one set of optional arrays: the call's chunks can be planned as a whole
  for (const BatchShape& b : bs) {
    total += b.batch;
    uniform = uniform && b.t_max == bs[0].t_max && b.k_sessions == bs[0].k_sessions && b.warm == bs[0].warm && b.want_y == bs[0].want_y;
  }
  std::vector<std::vector<Piece>> chunks;
  std::vector<long long> caps;
  long long fill = 0, cap = 0;
  const BatchShape* cur = nullptr;
  for (int g = 0; g < (int)bs.size(); ++g) {
    const BatchShape& b = bs[g];
    for (long long lo = 0; lo < b.batch;) {
      if (!cur || b.t_max != cur->t_max || b.k_sessions != cur->k_sessions || b.warm != cur->warm || b.want_y != cur->want_y || fill >= cap) {
        chunks.emplace_back();
        cur = &b; fill = 0;
        if (caps.empty() || !uniform) {
          // (the planner asks for the route of the CALL: under ACNQP_WAVE_MIN_BATCH a chunk may run another family)
          const acnqp::Route rt = acnqp::route_for(h->shape, b.t_max, b.k_sessions, (int)std::min<long long>(total, acnqp::kRouteAnyBatch), route_switches());
          acnqp::PlanEnv e = env;   // (env.direct: every batch of the call has a direct destination)
          e.direct = env.direct && rt.direct_x();
          caps = acnqp::plan_chunk_caps(total, rt.chunk_want(), acnqp::chunk_cap_by_memory((size_t)h->shape.N, (size_t)b.t_max, (size_t)b.k_sessions),
                                        rt.wv > 0, uniform, e);
        }
        cap = acnqp::chunk_cap(caps, chunks.size() - 1);
      }
      const long long n = std::min(b.batch - lo, cap - fill);
      chunks.back().push_back({g, lo, n, fill});
      fill += n; lo += n;
    }
  }
  return chunks;
}

// ---- fill: a chunk's inputs reach the slot's staging ------------------------------------------------------------------------
// Dense entry: the large arrays piece by piece, the small ones through the call's pinned mirror (hs; one H2D per chunk)
// or, without staging, a copy each; the chunks' input copies queue one chunk after the other (they share the link anyway:
// the first kernel's inputs do not wait for a share of the bandwidth the second chunk's copies would take).
int fill_dense(acnqp_handle* h, const Call& call, size_t c, const std::vector<Piece>& pcs, const ChunkLayout& L,
               acnqp_handle::Slot& S, char* hs) {
  const acnqp::SiteShape& s = h->shape;
  const BatchShape& b = call.bs[pcs[0].g];
  const size_t N = s.N, Tm = b.t_max, K = b.k_sessions, Mg = s.Mg, nv = N * Tm, ns = K * N;
  char* di = static_cast<char*>(S.in.p);
  static const bool chain = std::getenv("ACNQP_NO_H2D_CHAIN") == nullptr;
  if (chain && c > 0) HIP_TRY(hipStreamWaitEvent(S.st, h->h2d_done[(c - 1) % acnqp_handle::kSlots], 0));
  for (const Piece& pc : pcs) {
    const acnqp_problems& p = call.P[pc.g];
    const size_t lo = (size_t)pc.lo, n = (size_t)pc.n, pos = (size_t)pc.pos;
#define H2D(field, base, elem, per)                                                                             \
  HIP_TRY(hipMemcpyAsync(di + (base) + pos * (per) * (elem), reinterpret_cast<const char*>(p.field) + lo * (per) * (elem), \
                         n * (per) * (elem), hipMemcpyHostToDevice, S.st))
// small arrays: into the pinned mirror (one H2D per chunk below); without staging, a copy each
#define H2S(field, base, elem, per)                                                                             \
  do {                                                                                                          \
    if (hs) std::memcpy(hs + (base) + pos * (per) * (elem), reinterpret_cast<const char*>(p.field) + lo * (per) * (elem), n * (per) * (elem)); \
    else H2D(field, base, elem, per);                                                                           \
  } while (0)
    H2D(lb, L.lb, 8, nv);
    H2D(ub, L.ub, 8, nv);
    H2D(q, L.q, 8, nv);
    H2S(pdiag, L.pd, 8, 1);
    H2S(horizon, L.hz, 4, 1);
    H2S(s_off, L.so, 4, ns);
    H2S(s_len, L.sl, 4, ns);
    H2S(s_cap, L.sc, 8, ns);
    H2S(s_eq, L.eq, 1, 1);
    if (s.has_peak) H2S(peak, L.pk, 8, Tm);
    if (s.has_flat) H2S(lf, L.lf, 8, 1);
    if (s.has_max) { H2S(dc, L.dc, 8, 1); H2S(dfloor, L.df, 8, 1); }
    if (b.warm) { H2D(warm_x, L.wx, 8, nv); H2D(warm_y, L.wy, 8, Mg * Tm); }
    if (hs && L.xh != L.wx) {   // a direct chunk: where the kernel stores each problem's schedule (null: this piece is copied)
      double** tab = reinterpret_cast<double**>(hs + L.xh) + pos;
      double* const dst = call.xdst[pc.g];
      for (size_t i = 0; i < n; ++i) tab[i] = dst ? dst + (lo + i) * nv : nullptr;
    }
#undef H2S
#undef H2D
  }
  if (hs) HIP_TRY(hipMemcpyAsync(di + L.pd, hs + L.pd, L.wx - L.pd, hipMemcpyHostToDevice, S.st));
  if (chain) HIP_TRY(hipEventRecord(h->h2d_done[c % acnqp_handle::kSlots], S.st));
  return ACNQP_OK;
}

// Table entry: the chunk's slice of the session table into slot.tin, then table_expand_kernel forms lb, ub, q and the
// session slots in slot.in.
int fill_table(acnqp_handle* h, const Call& call, const Piece& pc, const ChunkLayout& L, const TableLayout& TL, acnqp_handle::Slot& S) {
  const acnqp::SiteShape& s = h->shape;
  const acnqp_table* T = call.T;
  const size_t N = s.N, Tm = T->t_max, K = T->k_sessions, nv = N * Tm;
  const long long lo = pc.lo, cn = pc.n, s0 = TL.s0, ns = TL.ns, r0 = TL.r0, nr = TL.nr;
  char* di = static_cast<char*>(S.in.p);
  char* dt = static_cast<char*>(S.tin.p);
#define TH2D(dst, src, bytes) do { if ((bytes) > 0) HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, S.st)); } while (0)
  TH2D(di + L.hz, T->horizon + lo, (size_t)cn * 4);
  TH2D(di + L.pd, T->pdiag + lo, (size_t)cn * 8);
  TH2D(di + L.eq, T->s_eq + lo, (size_t)cn);
  if (s.has_peak) TH2D(di + L.pk, T->peak + lo * Tm, (size_t)cn * Tm * 8);
  if (s.has_flat) TH2D(di + L.lf, T->lf + lo, (size_t)cn * 8);
  if (s.has_max) { TH2D(di + L.dc, T->dc + lo, (size_t)cn * 8); TH2D(di + L.df, T->dfloor + lo, (size_t)cn * 8); }
  TH2D(dt + TL.qi, T->q_index + lo, (size_t)cn * 4);
  TH2D(dt + TL.sg, T->sess_seg + lo, (size_t)(cn + 1) * 4);
  TH2D(dt + TL.ev, T->s_evse + s0, (size_t)ns * 4);
  TH2D(dt + TL.sl, T->s_slot + s0, (size_t)ns * 4);
  TH2D(dt + TL.of, T->s_off + s0, (size_t)ns * 4);
  TH2D(dt + TL.ln, T->s_len + s0, (size_t)ns * 4);
  TH2D(dt + TL.rs, T->rate_seg + s0, (size_t)(ns + 1) * 4);
  TH2D(dt + TL.cp, T->s_cap + s0, (size_t)ns * 8);
  TH2D(dt + TL.mn, T->min_rates + r0, (size_t)nr * 8);
  TH2D(dt + TL.mxr, T->max_rates + r0, (size_t)nr * 8);
  TH2D(dt + TL.qt, T->q_table, (size_t)T->n_horizons * nv * 8);
#undef TH2D
  TableExpandArgs ea;
  ea.N = (int)N; ea.Tm = (int)Tm; ea.K = (int)K; ea.s_base = s0; ea.r_base = r0;
  ea.q_index = reinterpret_cast<const int32_t*>(dt + TL.qi); ea.sess_seg = reinterpret_cast<const int32_t*>(dt + TL.sg);
  ea.s_evse = reinterpret_cast<const int32_t*>(dt + TL.ev); ea.s_slot = reinterpret_cast<const int32_t*>(dt + TL.sl);
  ea.s_off = reinterpret_cast<const int32_t*>(dt + TL.of); ea.s_len = reinterpret_cast<const int32_t*>(dt + TL.ln);
  ea.rate_seg = reinterpret_cast<const int32_t*>(dt + TL.rs); ea.q_table = reinterpret_cast<const double*>(dt + TL.qt);
  ea.s_cap = reinterpret_cast<const double*>(dt + TL.cp); ea.min_rates = reinterpret_cast<const double*>(dt + TL.mn);
  ea.max_rates = reinterpret_cast<const double*>(dt + TL.mxr);
  ea.lb = reinterpret_cast<double*>(di + L.lb); ea.ub = reinterpret_cast<double*>(di + L.ub); ea.q = reinterpret_cast<double*>(di + L.q);
  ea.so = reinterpret_cast<int32_t*>(di + L.so); ea.sl = reinterpret_cast<int32_t*>(di + L.sl); ea.sc = reinterpret_cast<double*>(di + L.sc);
  hipLaunchKernelGGL(table_expand_kernel, dim3((unsigned)cn), dim3(256), 0, S.st, ea);
  return ACNQP_OK;
}

// ---- the chunk loop ------------------------------------------------------------------------------------------------------
int run_call(acnqp_handle* h, Call& call, const acnqp_options* o) {
  const acnqp::SiteShape& s = h->shape;
  const size_t N = s.N, Mg = s.Mg;
  const bool table = call.T != nullptr;
  acnqp::PlanEnv env;
  if (const char* e = std::getenv("ACNQP_CHUNK")) env.chunk = std::atoll(e);
  env.plan = std::getenv("ACNQP_PLAN");
  static const bool ramp = std::getenv("ACNQP_NO_RAMP") == nullptr;
  env.ramp = ramp;
  // the direct path: the batches' destinations, asked once per batch (dense entry only)
  h->direct_x_last = 0;
  call.xdst.assign(call.bs.size(), nullptr);
  env.direct = !table && !call.bs.empty();
  for (size_t g = 0; g < call.bs.size() && !table; ++g) {
    call.xdst[g] = call.bs[g].batch > 0 ? direct_destination(call.R[g].x) : nullptr;
    env.direct = env.direct && (call.xdst[g] != nullptr || call.bs[g].batch == 0);
  }
  const std::vector<std::vector<Piece>> chunks = split_call(h, call.bs, env);
  // a chunk is direct if its launch's route can store to the host and one of its pieces has a destination
  std::vector<char> direct(chunks.size(), 0);
  for (size_t c = 0; c < chunks.size() && !table; ++c) {
    const std::vector<Piece>& pcs = chunks[c];
    const BatchShape& b = call.bs[pcs[0].g];
    if (!route_of(h, b.t_max, b.k_sessions, (int)(pcs.back().pos + pcs.back().n)).direct_x()) continue;
    for (const Piece& pc : pcs) direct[c] = direct[c] || call.xdst[pc.g] != nullptr;
  }
  auto layout = [&](size_t c) {
    const std::vector<Piece>& pcs = chunks[c];
    const BatchShape& b = call.bs[pcs[0].g];
    return ChunkLayout((size_t)(pcs.back().pos + pcs.back().n), N, b.t_max, b.k_sessions, Mg, s.has_peak, s.has_flat, s.has_max, b.warm, b.want_y,
                       direct[c] != 0);
  };
  // Dense entry only: pinned mirrors of the chunks' SMALL arrays (device ranges [pd, wx) and [st, y) of ChunkLayout),
  // whole call -- one H2D and one D2H per chunk instead of nine and five per piece; beyond kSmallCap the per-batch copies
  // of old (a call that large is not bound by their latency).  The table entry has neither the mirrors nor the H2D chain
  // of fill_dense: its small arrays keep a copy each, and it records and waits on no h2d_done event.  Giving it either
  // would change its speed, not its structure -- a change of its own, to be measured on its own.
  constexpr size_t kSmallCap = (size_t)256 << 20;
  std::vector<size_t> in_off(chunks.size()), out_off(chunks.size());
  size_t in_sum = 0, out_sum = 0;
  for (size_t c = 0; c < chunks.size() && !table; ++c) {
    const ChunkLayout L = layout(c);
    in_off[c] = in_sum; in_sum += L.wx - L.pd;
    out_off[c] = out_sum; out_sum += L.y - L.st;
  }
  static const bool no_stage = std::getenv("ACNQP_NO_STAGING") != nullptr;   // diagnostic: the per-batch copies
  const bool staged = !table && !no_stage && in_sum + out_sum <= kSmallCap;
  if (staged) {
    HIP_TRY(h->small_in.reserve(in_sum));
    HIP_TRY(h->small_out.reserve(out_sum));
  } else {
    std::fill(direct.begin(), direct.end(), 0);   // (the destinations ride in the mirror)
  }
  for (size_t c = 0; c < chunks.size(); ++c) {
    acnqp_handle::Slot& S = h->slot[c % acnqp_handle::kSlots];
    const std::vector<Piece>& pcs = chunks[c];   // (table entry: one piece)
    const BatchShape& b = call.bs[pcs[0].g];
    const size_t cn = (size_t)(pcs.back().pos + pcs.back().n), Tm = b.t_max;
    const ChunkLayout L = layout(c);
    const TableLayout TL = table ? TableLayout(call.T, pcs[0].lo, pcs[0].n, N * Tm) : TableLayout();
    if (L.in_total > S.in.cap || L.out_total > S.out.cap || TL.total > S.tin.cap) HIP_TRY(hipStreamSynchronize(S.st));   // staging still in use
    HIP_TRY(S.in.reserve(L.in_total));
    HIP_TRY(S.out.reserve(L.out_total));
    if (table) HIP_TRY(S.tin.reserve(TL.total));
    char* di = static_cast<char*>(S.in.p);
    char* dq = static_cast<char*>(S.out.p);
    char* hs = staged ? static_cast<char*>(h->small_in.p) + in_off[c] - L.pd : nullptr;    // hs + L.field = the mirror of di + L.field
    char* ho = staged ? static_cast<char*>(h->small_out.p) + out_off[c] - L.st : nullptr;  // ho + L.field = the mirror of dq + L.field
    // the ONE difference between the entries (see above for what the table entry deliberately does not share)
    int rc = table ? fill_table(h, call, pcs[0], L, TL, S) : fill_dense(h, call, c, pcs, L, S, hs);
    if (rc != ACNQP_OK) return rc;
    acnqp_problems dp;
    acnqp_results dr;
    device_views(L, di, dq, s, cn, b, &dp, &dr);
    double* const* x_host = direct[c] ? reinterpret_cast<double* const*>(di + L.xh) : nullptr;
    rc = solve_batch_device(h, &dp, o, &dr, S.st, c + 1 == chunks.size(), x_host);   // (the last chunk: nothing follows its launch)
    if (rc != ACNQP_OK) return rc;
    if (staged) HIP_TRY(hipMemcpyAsync(ho + L.st, dq + L.st, L.y - L.st, hipMemcpyDeviceToHost, S.st));
    for (const Piece& pc : pcs) {
      const acnqp_results& r = call.R[pc.g];
      const size_t lo = (size_t)pc.lo, n = (size_t)pc.n, pos = (size_t)pc.pos;
#define D2H(field, base, elem, per)                                                                          \
  HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(r.field) + lo * (per) * (elem), dq + (base) + pos * (per) * (elem), \
                         n * (per) * (elem), hipMemcpyDeviceToHost, S.st))
      if (direct[c] && call.xdst[pc.g]) h->direct_x_last += (long long)n;   // (the kernel has stored them, or will have)
      else D2H(x, L.x, 8, N * Tm);
      if (staged) {
        call.scatter.push_back(Scatter{pc.g, lo, n, pos, ho, L.st, L.it, L.pr, L.du, L.ob});
      } else {
        D2H(status, L.st, 4, 1);
        D2H(iters, L.it, 4, 1);
        D2H(pri_res, L.pr, 8, 1);
        D2H(dua_res, L.du, 8, 1);
        D2H(obj, L.ob, 8, 1);
      }
      if (b.want_y) D2H(y, L.y, 8, Mg * Tm);
#undef D2H
      if (r.x_dev)
        HIP_TRY(hipMemcpyAsync(r.x_dev + lo * N * Tm, dq + L.x + pos * N * Tm * 8, n * N * Tm * 8, hipMemcpyDeviceToDevice, S.st));
    }
  }
  return ACNQP_OK;
}

// ---- the epilogue of a host-buffer entry ------------------------------------------------------------------------------------
// run_call, then: drain every slot (also on failure: nothing may touch the caller's buffers afterwards), the ACNQP_TRACE
// line, the error mapping, the small result arrays out of the pinned mirror, and the scan for problems no kernel wrote.
// `who`: the entry's name in error texts; check_ms: time the entry spent checking its arguments (< 0: not reported).
int solve_call(acnqp_handle* h, Call& call, const acnqp_options* o, const char* who, double check_ms) {
  using clock = std::chrono::steady_clock;
  auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  static const bool trace = std::getenv("ACNQP_TRACE") != nullptr;   // diagnostic: check / enqueue / whole call, on stderr
  const auto t0 = clock::now();
  const int rc = run_call(h, call, o);
  const auto t1 = clock::now();
  hipError_t e = hipSuccess;
  for (auto& sl : h->slot) { const hipError_t e1 = hipStreamSynchronize(sl.st); if (e == hipSuccess) e = e1; }
  if (trace) {
    const auto t2 = clock::now();
    if (check_ms >= 0) std::fprintf(stderr, "[acnqp] %s: check %.3f ms, enqueue %.3f ms, drained after %.3f ms\n", who + 6, check_ms, ms(t0, t1), ms(t0, t2));
    else std::fprintf(stderr, "[acnqp] %s: enqueue %.3f ms, drained after %.3f ms\n", who + 6, ms(t0, t1), ms(t0, t2));
  }
  if (rc != ACNQP_OK) return rc;
  if (e != hipSuccess) return fail(ACNQP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  for (const Scatter& sc : call.scatter) {   // the small result arrays: pinned mirror -> the caller's arrays
    const acnqp_results& rr = call.R[sc.g];
    std::memcpy(rr.status + sc.lo, sc.host + sc.st + sc.pos * 4, sc.n * 4);
    std::memcpy(rr.iters + sc.lo, sc.host + sc.it + sc.pos * 4, sc.n * 4);
    std::memcpy(rr.pri_res + sc.lo, sc.host + sc.pr + sc.pos * 8, sc.n * 8);
    std::memcpy(rr.dua_res + sc.lo, sc.host + sc.du + sc.pos * 8, sc.n * 8);
    std::memcpy(rr.obj + sc.lo, sc.host + sc.ob + sc.pos * 8, sc.n * 8);
  }
  for (size_t g = 0; g < call.bs.size(); ++g)
    for (long long b = 0; b < call.bs[g].batch; ++b)
      if (call.R[g].status[b] == ACNQP_STATUS_UNSET)
        return fail(ACNQP_ERR_HIP, std::string(who) + ": " + (call.T ? "" : "batch " + std::to_string(g) + " ") + "problem " + std::to_string(b) +
                                   " was never written by the kernel (status UNSET after synchronisation): the launch did not execute completely");
  return ACNQP_OK;
}

}  // namespace
#endif  // __HIPCC__
