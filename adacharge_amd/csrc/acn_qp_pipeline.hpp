// The host-buffer entries' pipeline (acnqp_solve_batches, acnqp_solve_table): a call is cut into chunks that rotate
// over the handle's kSlots streams, so that the H2D copies, the kernels and the D2H copies of successive chunks overlap.
// ONE planner, ONE chunk loop and ONE epilogue for both entries; they differ in how a chunk's inputs reach the device
// (fill_dense / fill_table) and in nothing else.
//
// Part 1 (the tables of a chunk's arrays and of the session-table staging, their layouts, the planner) is plain host
// code: tests/test_chunk_layout.py and tests/test_route_table.py compile it with the host compiler.
// Part 2 (the kernels of this unit, the chunk loop) belongs to the API translation unit: acn_qp_api.hip includes this
// file after acnqp_handle, fail() and HIP_TRY.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "acn_qp.h"

namespace {
// the arguments of table_expand_kernel (Part 2); up here because the staging table of Part 1 names its pointer members
struct TableExpandArgs {
  int N, Tm, K;
  long long s_base, r_base;          // first session / rate entry of the chunk (the segment arrays hold global indices)
  const int32_t *q_index, *sess_seg, *s_evse, *s_slot, *s_off, *s_len, *rate_seg;
  const double *q_table, *s_cap, *min_rates, *max_rates;
  double *lb, *ub, *q, *sc;
  int32_t *so, *sl;
};
}  // namespace

namespace acnqp {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the arrays of a chunk: ONE table ----------------------------------------------------------------------------------
// A chunk of `cn` problems carries 16 input arrays (slot.in) and 7 result arrays (slot.out).  Each is one row below, and
// the layout, the device views, the copies in and out and the scatter of the small results all walk the rows: a new
// array is one row (and its name in the enum).  Rows stand in DEVICE order, every array on a 256-byte line.
struct ChunkShape {
  size_t N, Tm, K, Mg;
  bool peak, flat, max, warm, want_y, direct;
  bool direct_in = false;   // the chunk carries the host sources of its problems' lb / ub / q beside the destinations (row kXh)
};
enum class Per : uint8_t { One, NT, KN, T, MgT, Ptrs };                    // elements per problem
enum class When : uint8_t { Always, Peak, Flat, Max, Warm, WantY, Direct };  // the shapes that have the array
// Large: a copy per piece.  Small: rides in the call's pinned mirror, ONE copy per chunk and side (run_call), so the small
// rows of a side must stand together (static_assert below).
enum class Size : uint8_t { Large, Small };
constexpr size_t kNoField = ~(size_t)0;   // an array the library makes itself: no member of the ABI struct
struct ArrayRow { size_t field; uint8_t elem; Per per; When when; Size size; };   // field: offsetof in acnqp_problems / acnqp_results

enum In { kLb, kUb, kQ, kPd, kHz, kSo, kSl, kSc, kEq, kPk, kLf, kDc, kDf, kXh, kWx, kWy, kInRows };
enum Out { kX, kSt, kIt, kPr, kDu, kOb, kY, kOutRows };
constexpr ArrayRow kIn[kInRows] = {
    {offsetof(acnqp_problems, lb), 8, Per::NT, When::Always, Size::Large},
    {offsetof(acnqp_problems, ub), 8, Per::NT, When::Always, Size::Large},
    {offsetof(acnqp_problems, q), 8, Per::NT, When::Always, Size::Large},
    {offsetof(acnqp_problems, pdiag), 8, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_problems, horizon), 4, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_problems, s_off), 4, Per::KN, When::Always, Size::Small},
    {offsetof(acnqp_problems, s_len), 4, Per::KN, When::Always, Size::Small},
    {offsetof(acnqp_problems, s_cap), 8, Per::KN, When::Always, Size::Small},
    {offsetof(acnqp_problems, s_eq), 1, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_problems, peak), 8, Per::T, When::Peak, Size::Small},
    {offsetof(acnqp_problems, lf), 8, Per::One, When::Flat, Size::Small},
    {offsetof(acnqp_problems, dc), 8, Per::One, When::Max, Size::Small},
    {offsetof(acnqp_problems, dfloor), 8, Per::One, When::Max, Size::Small},
    // xh, the direct paths: where the kernel stores each problem's schedule (one double* per problem, filled by fill_dense)
    // and, in a chunk whose inputs the kernel loads itself (ChunkShape::direct_in), three more tables of cn pointers behind
    // that one: where it finds each problem's lb, ub and q (kHostLb ...: table k starts k * cn pointers into the row)
    {kNoField, sizeof(double*), Per::Ptrs, When::Direct, Size::Small},
    {offsetof(acnqp_problems, warm_x), 8, Per::NT, When::Warm, Size::Large},
    {offsetof(acnqp_problems, warm_y), 8, Per::MgT, When::Warm, Size::Large},
};
constexpr ArrayRow kOut[kOutRows] = {   // (acnqp_results::x_dev is a destination of x, not an array of the chunk)
    {offsetof(acnqp_results, x), 8, Per::NT, When::Always, Size::Large},
    {offsetof(acnqp_results, status), 4, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_results, iters), 4, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_results, pri_res), 8, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_results, dua_res), 8, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_results, obj), 8, Per::One, When::Always, Size::Small},
    {offsetof(acnqp_results, y), 8, Per::MgT, When::WantY, Size::Large},
};

constexpr bool present(const ArrayRow& r, const ChunkShape& s) {
  const bool on[] = {true, s.peak, s.flat, s.max, s.warm, s.want_y, s.direct || s.direct_in};   // (the order of When)
  return on[(int)r.when];
}
constexpr size_t bytes_per_problem(const ArrayRow& r, const ChunkShape& s) {
  const size_t n[] = {1, s.N * s.Tm, s.K * s.N, s.Tm, s.Mg * s.Tm, s.direct_in ? (size_t)4 : (size_t)1};   // (the order of Per)
  return r.elem * n[(int)r.per];
}
// the small rows of a side: [first, end), or {n, n} if they do not stand together
struct RowRange { int first, end; };
constexpr RowRange small_rows(const ArrayRow* rows, int n) {
  int first = 0, end = 0;
  while (first < n && rows[first].size != Size::Small) ++first;
  for (end = first; end < n && rows[end].size == Size::Small;) ++end;
  for (int k = end; k < n; ++k)
    if (rows[k].size == Size::Small) return {n, n};
  return {first, end};
}
enum HostTable { kHostX, kHostLb, kHostUb, kHostQ };   // the tables of row kXh
constexpr RowRange kSmallIn = small_rows(kIn, kInRows), kSmallOut = small_rows(kOut, kOutRows);
static_assert(kSmallIn.first < kSmallIn.end && kSmallOut.first < kSmallOut.end, "the small rows of a side are one contiguous run: the pinned mirror is one copy");

// device layout of one chunk of `cn` problems: in[k] / out[k] is where row k starts in slot.in / slot.out, in[kInRows] /
// out[kOutRows] the bytes of the side; an array the shape does not have takes no bytes
struct ChunkLayout {
  ChunkShape shape;
  size_t cn, in[kInRows + 1], out[kOutRows + 1];
  bool direct;   // the chunk carries the host destinations of its problems' schedules (kXh)
  bool direct_in;   // ... and the host sources of their lb / ub / q
  ChunkLayout(size_t cn_, const ChunkShape& s) : shape(s), cn(cn_), direct(s.direct), direct_in(s.direct_in) {
    auto lay = [&](const ArrayRow* rows, int n, size_t* off) {
      off[0] = 0;
      for (int k = 0; k < n; ++k) off[k + 1] = off[k] + al256(present(rows[k], s) ? cn * bytes_per_problem(rows[k], s) : 0);
    };
    lay(kIn, kInRows, in);
    lay(kOut, kOutRows, out);
  }
  // the device ranges that the pinned mirrors shadow: the small rows of each side
  size_t mirror_in() const { return in[kSmallIn.first]; }
  size_t mirror_in_bytes() const { return in[kSmallIn.end] - in[kSmallIn.first]; }
  size_t mirror_out() const { return out[kSmallOut.first]; }
  size_t mirror_out_bytes() const { return out[kSmallOut.end] - out[kSmallOut.first]; }
  size_t host_table(HostTable k) const { return in[kXh] + (size_t)k * cn * sizeof(double*); }   // (k > kHostX: direct_in chunks only)
};

// ---- the session-table staging: ONE table -------------------------------------------------------------------------------
// What fill_table uploads into slot.tin for the chunk of problems [lo, lo + cn): their ns sessions from s0 on and those
// sessions' nr rate entries from r0 on (sess_seg / rate_seg hold global indices), and the whole q_table.
struct TableSpan { long long lo = 0, cn = 0, s0 = 0, ns = 0, r0 = 0, nr = 0; size_t qt = 0; };   // qt: elements of q_table, H N Tm
enum class Count : uint8_t { Cn, Cn1, Ns, Ns1, Nr, Qt };
enum class Base : uint8_t { Lo, S0, R0, Zero };
struct TableRow { size_t field, arg; uint8_t elem; Count count; Base base; };   // field: offsetof in acnqp_table, arg: in TableExpandArgs
#define ACNQP_T(f) offsetof(acnqp_table, f), offsetof(TableExpandArgs, f)   // (the two structs name an array alike)
constexpr TableRow kTable[] = {
    {ACNQP_T(q_index), 4, Count::Cn, Base::Lo},
    {ACNQP_T(sess_seg), 4, Count::Cn1, Base::Lo},
    {ACNQP_T(s_evse), 4, Count::Ns, Base::S0},
    {ACNQP_T(s_slot), 4, Count::Ns, Base::S0},
    {ACNQP_T(s_off), 4, Count::Ns, Base::S0},
    {ACNQP_T(s_len), 4, Count::Ns, Base::S0},
    {ACNQP_T(rate_seg), 4, Count::Ns1, Base::S0},
    {ACNQP_T(s_cap), 8, Count::Ns, Base::S0},
    {ACNQP_T(min_rates), 8, Count::Nr, Base::R0},
    {ACNQP_T(max_rates), 8, Count::Nr, Base::R0},
    {ACNQP_T(q_table), 8, Count::Qt, Base::Zero},
};
#undef ACNQP_T
constexpr int kTableRows = (int)(sizeof(kTable) / sizeof(kTable[0]));
constexpr size_t table_count(const TableRow& r, const TableSpan& s) {   // elements uploaded ...
  const size_t n[] = {(size_t)s.cn, (size_t)s.cn + 1, (size_t)s.ns, (size_t)s.ns + 1, (size_t)s.nr, s.qt};
  return n[(int)r.count];
}
constexpr size_t table_base(const TableRow& r, const TableSpan& s) {   // ... from this element of the caller's array on
  const long long at[] = {s.lo, s.s0, s.r0, 0};
  return (size_t)at[(int)r.base];
}
struct TableLayout {
  TableSpan span;
  size_t off[kTableRows] = {}, total = 0;
  TableLayout() = default;   // (dense entry: no table staging)
  explicit TableLayout(const TableSpan& s) : span(s) {
    for (int k = 0; k < kTableRows; ++k) { off[k] = total; total += al256(table_count(kTable[k], s) * kTable[k].elem); }
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
  bool direct_in = false;       // not a variable: the kernel loads lb / ub / q of the call's first problems from the caller's host
                                // arrays (Route::direct_in, run_call), so the first launch waits for the small arrays only.  Under
                                // this flag alone may a plan differ from the one without it; none does today
};

// inputs + results staged per problem -- every one of the kSlots pipeline slots holds a chunk of each, so a chunk is
// capped at 1 GiB of the sum.  (The kernels' workspaces belong to the resident workgroup slots: no per-problem term.)
// The formula APPROXIMATES the byte sum of the table above (lb, ub, q, x; the session slots; peak; 96 bytes of scalars) and
// ignores the warm-start and y arrays.  Kept, not derived from the table: its values are the chunk sizes (test_route_table.py).
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

using namespace acnqp;   // the tables of Part 1

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

// ---- a call and its chunks ---------------------------------------------------------------------------------------------
struct BatchShape { long long batch; int t_max, k_sessions; bool warm, want_y; };
struct Piece { int g; long long lo, n, pos; };   // problems [lo, lo + n) of batch g sit at [pos, pos + n) of their chunk
// what the caller's small result arrays still need after the streams have drained, a copy out of the pinned mirror: the
// piece, its chunk, and the mirror base (host + layout[c].out[k] is the mirror of row k)
struct Scatter { Piece pc; size_t c; const char* host; };

// one call of a host-buffer entry: dense batches P[nb] (acnqp_solve_batches) or ONE session table T (acnqp_solve_table)
struct Call {
  const acnqp_problems* P = nullptr;
  const acnqp_table* T = nullptr;
  acnqp_results* R = nullptr;      // [nb]; the table's one
  std::vector<BatchShape> bs;
  std::vector<ChunkLayout> layout; // [chunk], as run_call reaches them
  std::vector<Scatter> scatter;    // dense entry with staged small arrays
  std::vector<double*> xdst;       // [nb] the direct path: R[g].x as the device addresses it (null: batch g keeps its copies)
  struct HostIn { const double *lb = nullptr, *ub = nullptr, *q = nullptr; };
  std::vector<HostIn> isrc;        // [nb] the direct path for the inputs: P[g].lb / ub / q as the device addresses them (all
                                   // three, or none: batch g keeps its copies); asked of the leading chunk's batches only
};

// ---- the direct path for x ---------------------------------------------------------------------------------------------
// A result array x in device-addressable host memory (pinned: acnqp_host_alloc, hipHostMalloc, hipHostRegister) is written
// by the kernel itself where the route can do that (Route::direct_x; TiledArgs::x_host): the wave that gives a problem
// its verdict stores the schedule there, pol_x_to_host_kernel (acn_qp_api.hip) those of the handed-over problems, and the
// chunk loop queues no copy of x.  The destinations ride with the chunk's small inputs (row kXh), so only the
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

// ---- the direct path for lb / ub / q --------------------------------------------------------------------------------------
// The mirror image, for the call's LEADING chunk only: nothing overlaps the copy of the first chunk's inputs, and the
// wave kernel reads every value of lb / ub / q exactly once, at problem start.  Where the route can do that
// (Route::direct_in; TiledArgs::lb_host ...) and a batch's lb, ub and q are ALL in device-addressable host memory, the
// chunk loop queues no copy of the three for that batch's piece of chunk 0 -- in a call of several chunks; a call of one
// chunk keeps its copies (run_call) --: the first launch starts once the small arrays have landed, its waves fetch the values over the link and complete the chunk's device copy as they go (the retry
// passes, the polish, the resume launch and the dual report read it), and the next chunk's copies start at once beside
// it.  The sources ride with the chunk's small inputs (row kXh, tables kHostLb ...), so only the dense entry with its
// pinned mirrors takes the path; decided per piece, so a call may mix pinned and pageable batches.  The chunk takes the
// session-count launch order: the congestion key reads ub, which is not on the device when it would run.  Every later
// chunk, the table entry and the device entry are as they were.
// ACNQP_NO_DIRECT_IN=1 (diagnostic, read once per process): the copies everywhere.
const double* direct_source(const double* a) {
  static const bool off = std::getenv("ACNQP_NO_DIRECT_IN") != nullptr;
  if (off || a == nullptr) return nullptr;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, a) != hipSuccess) {   // (memory the runtime does not know: pageable)
    (void)hipGetLastError();
    return nullptr;
  }
  return at.type == hipMemoryTypeHost ? static_cast<const double*>(at.devicePointer) : nullptr;
}

// the pointer member at byte `field` of an ABI struct (every member the tables name is a pointer to objects)
inline char* member(const void* s, size_t field) { char* p; std::memcpy(&p, static_cast<const char*>(s) + field, sizeof p); return p; }
inline void set_member(void* s, size_t field, const void* p) { std::memcpy(static_cast<char*>(s) + field, &p, sizeof p); }

// the device-side view of the chunk laid out by L in a slot's staging (di: inputs, dq: results); null for an array the
// chunk's shape does not have
void device_views(const ChunkLayout& L, char* di, char* dq, const BatchShape& b, acnqp_problems* dp, acnqp_results* dr) {
  dp->batch = (int32_t)L.cn; dp->t_max = b.t_max; dp->k_sessions = b.k_sessions;
  for (int k = 0; k < kInRows; ++k)
    if (kIn[k].field != kNoField) set_member(dp, kIn[k].field, present(kIn[k], L.shape) ? di + L.in[k] : nullptr);
  for (int k = 0; k < kOutRows; ++k) set_member(dr, kOut[k].field, present(kOut[k], L.shape) ? dq + L.out[k] : nullptr);
  dr->x_dev = nullptr;
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
          e.direct_in = env.direct_in && rt.direct_in();
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
// Problems [lo, lo + n) of the host arrays `src` to [pos, pos + n) of the chunk, row by row: a large row is a copy on st,
// a small row goes into the pinned mirror hs (hs + L.in[k] mirrors di + L.in[k]; null: no mirror, a copy each).  A row
// without a source (kXh; the arrays that table_expand_kernel forms) is not the caller's to copy, and `loaded` says that the
// kernel loads this piece's lb / ub / q itself (the direct path for the inputs).
hipError_t upload_piece(const ChunkLayout& L, const acnqp_problems& src, size_t lo, size_t n, size_t pos, char* di, char* hs, hipStream_t st,
                        bool loaded = false) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < kInRows && e == hipSuccess; ++k) {
    const char* from = kIn[k].field != kNoField && present(kIn[k], L.shape) ? member(&src, kIn[k].field) : nullptr;
    if (!from || (loaded && (k == kLb || k == kUb || k == kQ))) continue;
    const size_t per = bytes_per_problem(kIn[k], L.shape);
    if (hs && kIn[k].size == Size::Small) std::memcpy(hs + L.in[k] + pos * per, from + lo * per, n * per);
    else e = hipMemcpyAsync(di + L.in[k] + pos * per, from + lo * per, n * per, hipMemcpyHostToDevice, st);
  }
  return e;
}

// Dense entry: the large arrays piece by piece, the small ones through the call's pinned mirror (hs; one H2D per chunk)
// or, without staging, a copy each; the chunks' input copies queue one chunk after the other (they share the link anyway:
// the first kernel's inputs do not wait for a share of the bandwidth the second chunk's copies would take).
int fill_dense(acnqp_handle* h, const Call& call, size_t c, const std::vector<Piece>& pcs, const ChunkLayout& L,
               acnqp_handle::Slot& S, char* hs) {
  char* di = static_cast<char*>(S.in.p);
  static const bool chain = std::getenv("ACNQP_NO_H2D_CHAIN") == nullptr;
  if (chain && c > 0) HIP_TRY(hipStreamWaitEvent(S.st, h->h2d_done[(c - 1) % acnqp_handle::kSlots], 0));
  for (const Piece& pc : pcs) {
    const size_t lo = (size_t)pc.lo, n = (size_t)pc.n, pos = (size_t)pc.pos;
    const Call::HostIn in = hs && L.direct_in ? call.isrc[pc.g] : Call::HostIn();   // (all three, or none)
    HIP_TRY(upload_piece(L, call.P[pc.g], lo, n, pos, di, hs, S.st, in.lb != nullptr));
    const size_t nv = L.shape.N * L.shape.Tm;
    if (hs && (L.direct || L.direct_in)) {   // where the kernel stores each problem's schedule (null: this piece is copied)
      double** tab = reinterpret_cast<double**>(hs + L.host_table(kHostX)) + pos;
      double* const dst = L.direct ? call.xdst[pc.g] : nullptr;
      for (size_t i = 0; i < n; ++i) tab[i] = dst ? dst + (lo + i) * nv : nullptr;
    }
    if (hs && L.direct_in) {   // where it finds each problem's lb, ub and q (null: this piece was copied)
      const double* const from[] = {in.lb, in.ub, in.q};
      const HostTable which[] = {kHostLb, kHostUb, kHostQ};
      for (int k = 0; k < 3; ++k) {
        const double** tab = reinterpret_cast<const double**>(hs + L.host_table(which[k])) + pos;
        for (size_t i = 0; i < n; ++i) tab[i] = from[k] ? from[k] + (lo + i) * nv : nullptr;
      }
    }
  }
  if (hs) HIP_TRY(hipMemcpyAsync(di + L.mirror_in(), hs + L.mirror_in(), L.mirror_in_bytes(), hipMemcpyHostToDevice, S.st));
  if (chain) HIP_TRY(hipEventRecord(h->h2d_done[c % acnqp_handle::kSlots], S.st));
  return ACNQP_OK;
}

// the chunk of problems [lo, lo + cn) of a session table: its sessions and their rate entries
TableSpan table_span(const acnqp_table* T, long long lo, long long cn, size_t nv) {
  const long long s0 = T->sess_seg[lo], ns = T->sess_seg[lo + cn] - s0, r0 = T->rate_seg[s0], nr = T->rate_seg[s0 + ns] - r0;
  return TableSpan{lo, cn, s0, ns, r0, nr, (size_t)T->n_horizons * nv};
}

// Table entry: the per-problem arrays that the table has (a copy each), the chunk's slice of the session table into
// slot.tin, then table_expand_kernel forms lb, ub, q and the session slots in slot.in.
int fill_table(const Call& call, const Piece& pc, const ChunkLayout& L, const TableLayout& TL, acnqp_handle::Slot& S) {
  const acnqp_table* T = call.T;
  char* di = static_cast<char*>(S.in.p);
  char* dt = static_cast<char*>(S.tin.p);
  acnqp_problems src = {};
  src.horizon = T->horizon; src.pdiag = T->pdiag; src.s_eq = T->s_eq; src.peak = T->peak; src.lf = T->lf; src.dc = T->dc; src.dfloor = T->dfloor;
  HIP_TRY(upload_piece(L, src, (size_t)pc.lo, (size_t)pc.n, 0, di, nullptr, S.st));
  TableExpandArgs ea;
  for (int k = 0; k < kTableRows; ++k) {
    const TableRow& r = kTable[k];
    const size_t bytes = table_count(r, TL.span) * r.elem;
    if (bytes > 0) HIP_TRY(hipMemcpyAsync(dt + TL.off[k], member(T, r.field) + table_base(r, TL.span) * r.elem, bytes, hipMemcpyHostToDevice, S.st));
    set_member(&ea, r.arg, dt + TL.off[k]);
  }
  ea.N = (int)L.shape.N; ea.Tm = (int)L.shape.Tm; ea.K = (int)L.shape.K; ea.s_base = TL.span.s0; ea.r_base = TL.span.r0;
  ea.lb = reinterpret_cast<double*>(di + L.in[kLb]); ea.ub = reinterpret_cast<double*>(di + L.in[kUb]); ea.q = reinterpret_cast<double*>(di + L.in[kQ]);
  ea.so = reinterpret_cast<int32_t*>(di + L.in[kSo]); ea.sl = reinterpret_cast<int32_t*>(di + L.in[kSl]); ea.sc = reinterpret_cast<double*>(di + L.in[kSc]);
  hipLaunchKernelGGL(table_expand_kernel, dim3((unsigned)pc.n), dim3(256), 0, S.st, ea);
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
  // the direct path for the inputs: the sources of a batch, asked once per batch and call and only of the batches that
  // reach into the leading chunk (all three arrays, or the batch keeps its copies)
  h->direct_in_last = 0;
  call.isrc.assign(call.bs.size(), Call::HostIn());
  std::vector<char> asked(call.bs.size(), 0);
  auto sources = [&](int g) {
    if (!asked[g]) {
      asked[g] = 1;
      const acnqp_problems& P = call.P[g];
      Call::HostIn in;
      in.lb = direct_source(P.lb);
      if (in.lb) in.ub = direct_source(P.ub);
      if (in.ub) in.q = direct_source(P.q);
      if (in.q) call.isrc[g] = in;
    }
    return call.isrc[g].lb != nullptr;
  };
  for (size_t g = 0; g < call.bs.size() && !table; ++g)   // the planner's flag: the call's first problem comes that way
    if (call.bs[g].batch > 0) { env.direct_in = sources((int)g); break; }
  const std::vector<std::vector<Piece>> chunks = split_call(h, call.bs, env);
  // chunk 0 of a call of several chunks, where its launch's route can load from the host and one of its pieces has sources.
  // (A call of ONE chunk keeps its copies: nothing runs beside its first launch that the fetch could make room for, and 256
  // waves fetching 4 MB measured slower than the copy -- the strict batch-256 call 2.852-2.864 -> 2.911-2.930 ms, a loss by
  // the rule, profiles/direct_in_ab_one_chunk_calls.json.)
  bool direct_in = false;
  if (!table && chunks.size() > 1) {
    const std::vector<Piece>& pcs = chunks[0];
    const BatchShape& b = call.bs[pcs[0].g];
    if (route_of(h, b.t_max, b.k_sessions, (int)(pcs.back().pos + pcs.back().n)).direct_in())
      for (const Piece& pc : pcs) direct_in = sources(pc.g) || direct_in;
  }
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
    return ChunkLayout((size_t)(pcs.back().pos + pcs.back().n),
                       ChunkShape{N, (size_t)b.t_max, (size_t)b.k_sessions, Mg, s.has_peak != 0, s.has_flat != 0, s.has_max != 0, b.warm, b.want_y, direct[c] != 0,
                                  direct_in && c == 0});
  };
  // Dense entry only: pinned mirrors of the chunks' SMALL arrays (ChunkLayout::mirror_in / mirror_out: the small rows of
  // the table), whole call -- one H2D and one D2H per chunk instead of nine and five per piece; beyond kSmallCap the per-batch
  // copies of old (a call that large is not bound by their latency).  The table entry has neither the mirrors nor the H2D
  // chain of fill_dense: its small arrays keep a copy each, and it records and waits on no h2d_done event.  Giving it either
  // would change its speed, not its structure -- a change of its own, to be measured on its own.
  constexpr size_t kSmallCap = (size_t)256 << 20;
  std::vector<size_t> in_off(chunks.size()), out_off(chunks.size());
  size_t in_sum = 0, out_sum = 0;
  for (size_t c = 0; c < chunks.size() && !table; ++c) {
    const ChunkLayout L = layout(c);
    in_off[c] = in_sum; in_sum += L.mirror_in_bytes();
    out_off[c] = out_sum; out_sum += L.mirror_out_bytes();
  }
  static const bool no_stage = std::getenv("ACNQP_NO_STAGING") != nullptr;   // diagnostic: the per-batch copies
  const bool staged = !table && !no_stage && in_sum + out_sum <= kSmallCap;
  if (staged) {
    HIP_TRY(h->small_in.reserve(in_sum));
    HIP_TRY(h->small_out.reserve(out_sum));
  } else {
    std::fill(direct.begin(), direct.end(), 0);   // (the destinations and the sources ride in the mirror)
    direct_in = false;
  }
  for (size_t c = 0; c < chunks.size(); ++c) {
    acnqp_handle::Slot& S = h->slot[c % acnqp_handle::kSlots];
    const std::vector<Piece>& pcs = chunks[c];   // (table entry: one piece)
    const BatchShape& b = call.bs[pcs[0].g];
    call.layout.push_back(layout(c));
    const ChunkLayout& L = call.layout.back();
    const TableLayout TL = table ? TableLayout(table_span(call.T, pcs[0].lo, pcs[0].n, N * L.shape.Tm)) : TableLayout();
    HIP_TRY(reserve_behind(S.st, {{&S.in, L.in[kInRows]}, {&S.out, L.out[kOutRows]}, {&S.tin, TL.total}}));
    char* di = static_cast<char*>(S.in.p);
    char* dq = static_cast<char*>(S.out.p);
    char* hs = staged ? static_cast<char*>(h->small_in.p) + in_off[c] - L.mirror_in() : nullptr;     // hs + L.in[k] = the mirror of di + L.in[k]
    char* ho = staged ? static_cast<char*>(h->small_out.p) + out_off[c] - L.mirror_out() : nullptr;  // ho + L.out[k] = the mirror of dq + L.out[k]
    // the ONE difference between the entries (see above for what the table entry deliberately does not share)
    int rc = table ? fill_table(call, pcs[0], L, TL, S) : fill_dense(h, call, c, pcs, L, S, hs);
    if (rc != ACNQP_OK) return rc;
    acnqp_problems dp;
    acnqp_results dr;
    device_views(L, di, dq, b, &dp, &dr);
    HostTables ht;
    if (L.direct) ht.x = reinterpret_cast<double* const*>(di + L.host_table(kHostX));
    if (L.direct_in) {
      ht.lb = reinterpret_cast<const double* const*>(di + L.host_table(kHostLb));
      ht.ub = reinterpret_cast<const double* const*>(di + L.host_table(kHostUb));
      ht.q = reinterpret_cast<const double* const*>(di + L.host_table(kHostQ));
    }
    rc = solve_batch_device(h, &dp, o, &dr, S.st, c + 1 == chunks.size(), ht);   // (the last chunk: nothing follows its launch)
    if (rc != ACNQP_OK) return rc;
    if (staged) HIP_TRY(hipMemcpyAsync(ho + L.mirror_out(), dq + L.mirror_out(), L.mirror_out_bytes(), hipMemcpyDeviceToHost, S.st));
    for (const Piece& pc : pcs) {
      const acnqp_results& r = call.R[pc.g];
      const size_t lo = (size_t)pc.lo, n = (size_t)pc.n, pos = (size_t)pc.pos;
      const bool stored = L.direct && call.xdst[pc.g];   // (the kernel has stored this piece's x, or will have)
      if (stored) h->direct_x_last += (long long)n;
      if (L.direct_in && call.isrc[pc.g].lb) h->direct_in_last += (long long)n;
      for (int k = 0; k < kOutRows; ++k) {   // a copy each, but: x of a stored piece, the small rows of a staged call
        if (!present(kOut[k], L.shape) || (k == kX && stored) || (staged && kOut[k].size == Size::Small)) continue;
        const size_t per = bytes_per_problem(kOut[k], L.shape);
        HIP_TRY(hipMemcpyAsync(member(&r, kOut[k].field) + lo * per, dq + L.out[k] + pos * per, n * per, hipMemcpyDeviceToHost, S.st));
      }
      if (staged) call.scatter.push_back(Scatter{pc, c, ho});
      if (r.x_dev) {
        const size_t per = bytes_per_problem(kOut[kX], L.shape);
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(r.x_dev) + lo * per, dq + L.out[kX] + pos * per, n * per, hipMemcpyDeviceToDevice, S.st));
      }
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
    const ChunkLayout& L = call.layout[sc.c];
    for (int k = kSmallOut.first; k < kSmallOut.end; ++k) {
      const size_t per = bytes_per_problem(kOut[k], L.shape);
      std::memcpy(member(&call.R[sc.pc.g], kOut[k].field) + (size_t)sc.pc.lo * per, sc.host + L.out[k] + (size_t)sc.pc.pos * per, (size_t)sc.pc.n * per);
    }
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
