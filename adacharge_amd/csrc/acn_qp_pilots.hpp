// Pilot signals (acnqp_pilots_device / acnqp_pilots_host, include/acn_qp.h): what the reference does to a solved schedule
// before it goes to the chargers (ada.py:176-189), for a whole batch on the device.  Three modes:
//
//   CONTINUOUS  max(min(x, max_pilot_i), 0)                                                   post.py:77-94
//   DISCRETE    max(floor_to_set(x, levels_i, 0.05), 0), every entry, padding periods included post.py:97-118
//   REALLOCATE  DISCRETE, then the greedy round robin of post.py:189-258 on period 0: the EVSEs are visited in the
//               order of their rounding loss; a visit raises the EVSE to its next level when the aggregate stays
//               under the solved period's, the EVSE under its cap and the network feasible, and retires it otherwise
//
// tests/pilots_spec.py states all three in plain numpy loops; the kernel is held to it BIT FOR BIT.  That is possible
// because every operation is an IEEE-754 double add, multiply or comparison in a stated order:
//   * floor_to_set is a count, pos = #{k : levels[k] < x + 0.05} (comparisons only)
//   * the visiting order is (rank of the EVSE's key, session index): comparisons only.  It is never materialised: the
//     next visit is the smallest (rank, session) code behind the current one among the sessions of active EVSEs, found
//     by a wavefront minimum -- so an EVSE may carry any number of sessions (it is visited once per session and
//     cycle, as in the reference) and nothing has a capacity
//   * the sums of the acceptance test run over the EVSEs in increasing order inside ONE lane (lane = infrastructure
//     row, lane M = the aggregate), every product and every sum rounded once: contraction is switched off inside the
//     kernel, and the row test compares squares (no sqrt, no hypot)
// The loop is a counted loop: a problem makes at most N L active visits (each is an increment or a retirement); one
// whose last level lies below a cap never retires (the reference spins for ever) and is reported as visits = -1.
//
// One workgroup per problem, its size chosen by the shape only (pilots_threads): ONE wavefront for N <= 64, four
// beyond.  All threads stream the (N, Tm) body and stage period 0, caps, ranks and -- where they fit
// (pilots_layout, shape only) -- the site's rows and the level table in LDS; the first wavefront then runs the round
// robin alone (wavefront-scope fences, no workgroup barrier inside the loop).  No atomics; every output element is
// written whatever the input; a problem gives the same bits alone and at any position of any batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace acnqp {

constexpr int kPilotsContinuous = 0, kPilotsDiscrete = 1, kPilotsReallocate = 2;

struct PilotsArgs {
  int B, N, Tm, M, L, mode;
  const double *cre, *cim;   // [M][N] real / imaginary part of the site rows (utils.py:5-12: always the SOC form)
  const double* limits;      // [M]
  const double* max_pilot;   // [N]
  const double* levels;      // [N][L] ascending, padded with +inf
  const int32_t* sess_seg;   // [B + 1]
  const int32_t* s_evse;     // [S]
  const uint8_t* s_arrived;  // [S] arrival_offset == 0 and a non-empty window
  const double* s_cap;       // [S] first-period cap of an arrived session
  const double* x;           // [B][N][Tm]
  double* pilots;            // [B][N][Tm] or nullptr
  double* first;             // [B][N] or nullptr
  int32_t* visits;           // [B] or nullptr
  int site_lds, levels_lds;  // pilots_layout: what is staged in LDS
};

// LDS of one workgroup, a function of the shape only: per-EVSE state always; the site rows and the level table when
// the whole stays within the 64 KB a launch gets without asking
struct PilotsLayout {
  int site_lds, levels_lds;
  size_t bytes;
};
inline PilotsLayout pilots_layout(int N, int M, int L, int mode) {
  PilotsLayout p{0, 0, 0};
  const size_t budget = 60 * 1024;
  size_t need = mode == kPilotsReallocate ? (size_t)N * (3 * 8 + 2 * 4) + (size_t)(M + 2) * 8 : 0;
  const size_t site = (size_t)2 * M * N * 8, lev = (size_t)N * L * 8;
  if (mode == kPilotsReallocate && M > 0 && need + site <= budget) { p.site_lds = 1; need += site; }
  if (mode != kPilotsContinuous && need + lev <= budget) { p.levels_lds = 1; need += lev; }
  p.bytes = (need + 15) & ~(size_t)15;
  return p;
}
inline int pilots_threads(int N) { return N <= 64 ? 64 : 256; }

constexpr double kPilotsInf = __builtin_huge_val();
constexpr double kPilotsEps = 0.05;        // post.py:10-31
constexpr double kPilotsSlack = 1e-7;      // utils.py:5-12
constexpr unsigned long long kPilotsNone = ~0ull, kPilotsWrap = 1ull << 62;

// max(floor_to_set(x, levels, 0.05), 0): pos = #{k : levels[k] < x + 0.05}; level pos - 1, the first one for pos == 0
__device__ inline double pilots_floor(double x, const double* lv, int L) {
#pragma clang fp contract(off)
  const double xe = x + kPilotsEps;
  int pos = 0;
  for (int k = 0; k < L; ++k) pos += lv[k] < xe ? 1 : 0;
  const double v = lv[pos > 0 ? pos - 1 : 0];
  return v >= 0.0 ? v : 0.0;
}
__device__ inline double pilots_clip(double x, double cap) {
  const double v = x <= cap ? x : cap;
  return v >= 0.0 ? v : 0.0;
}

__device__ inline unsigned long long pilots_wave_min(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}
// orders this wavefront's LDS writes before its later LDS reads (other lanes' included): one wavefront executes its
// LDS instructions in order, the fences keep the compiler from moving them
__device__ inline void pilots_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void pilots_kernel(const PilotsArgs A) {
#pragma clang fp contract(off)   // every product and every sum of this kernel is rounded once (tests/pilots_spec.py)
  extern __shared__ __attribute__((aligned(16))) char pilots_lds[];
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int N = A.N, Tm = A.Tm, M = A.M, L = A.L;
  const int n = N * Tm;   // (N <= 1024, Tm <= 4096: 32-bit index arithmetic inside a problem)
  const double* x = A.x + (size_t)b * n;
  double* po = A.pilots ? A.pilots + (size_t)b * n : nullptr;
  double* fo = A.first ? A.first + (size_t)b * N : nullptr;
  const bool realloc = A.mode == kPilotsReallocate;

  // ---- LDS carve (pilots_layout) ----------------------------------------------------------------------------------
  double* x0 = reinterpret_cast<double*>(pilots_lds);   // [N] period 0 as solved
  double* col = x0 + (realloc ? N : 0);                 // [N] period 0 of the pilots
  double* cap = col + (realloc ? N : 0);                // [N]
  double* lim2 = cap + (realloc ? N : 0);               // [M + 2]: (limit + 1e-7)^2 per row
  double* sre = lim2 + (realloc ? M + 2 : 0);           // [N][M] site rows, EVSE-major (lane = row reads neighbours)
  double* sim = sre + (A.site_lds ? (size_t)M * N : 0);
  double* slv = sim + (A.site_lds ? (size_t)M * N : 0); // [N][L]
  int* rank = reinterpret_cast<int*>(slv + (A.levels_lds ? (size_t)N * L : 0));   // [N]
  int* active = rank + (realloc ? N : 0);                                           // [N]
  const double* lv = A.levels_lds ? slv : A.levels;
  if (A.levels_lds) {
    for (int k = gt; k < N * L; k += THREADS) slv[k] = A.levels[k];
    __syncthreads();
  }

  // ---- the body: every entry but (REALLOCATE) period 0, which the round robin writes ---------------------------------
  if (po) {
    for (int k = gt; k < n; k += THREADS) {
      const int i = k / Tm;
      if (realloc && k == i * Tm) continue;
      po[k] = A.mode == kPilotsContinuous ? pilots_clip(x[k], A.max_pilot[i]) : pilots_floor(x[k], lv + (size_t)i * L, L);
    }
  }
  if (!realloc) {
    for (int i = gt; i < N; i += THREADS) {
      const double xv = x[(size_t)i * Tm];
      const double v = A.mode == kPilotsContinuous ? pilots_clip(xv, A.max_pilot[i]) : pilots_floor(xv, lv + (size_t)i * L, L);
      if (fo) fo[i] = v;
    }
    if (gt == 0 && A.visits) A.visits[b] = 0;
    return;
  }

  // ---- REALLOCATE: period 0, caps and the site into LDS ---------------------------------------------------------------
  const int seg0 = A.sess_seg[b];
  const int Sb = A.sess_seg[b + 1] - seg0 > 0 ? A.sess_seg[b + 1] - seg0 : 0;
  const int32_t* sev = A.s_evse + seg0;
  for (int i = gt; i < N; i += THREADS) {
    const double xv = x[(size_t)i * Tm];
    x0[i] = xv;
    col[i] = pilots_floor(xv, lv + (size_t)i * L, L);
    int act = 0;
    double c = 0.0;
    for (int s = 0; s < Sb; ++s)   // one arrived session per EVSE; a later one overwrites, as the reference's loop does
      if (sev[s] == i && A.s_arrived[seg0 + s]) { act = 1; c = A.s_cap[seg0 + s]; }
    active[i] = act;
    cap[i] = c;
  }
  for (int j = gt; j < M; j += THREADS) {
    const double t = A.limits[j] + kPilotsSlack;
    lim2[j] = t * t;
  }
  if (A.site_lds)
    for (int k = gt; k < M * N; k += THREADS) {
      const int j = k / N, i = k - j * N;
      sre[(size_t)i * M + j] = A.cre[k];
      sim[(size_t)i * M + j] = A.cim[k];
    }
  __syncthreads();
  // rank of the EVSE's key -(x0 - rounded) among the EVSEs (equal keys share a rank): the visiting order is
  // (rank, session index), the stable sort of the sessions by their EVSE's key
  for (int i = gt; i < N; i += THREADS) {
    const double key = -(x0[i] - col[i]);
    int r = 0;
    for (int k = 0; k < N; ++k) r += -(x0[k] - col[k]) < key ? 1 : 0;
    rank[i] = r;
  }
  __syncthreads();
  if (gt >= 64) return;   // the round robin is sequential: the first wavefront runs it alone

  const int lane = gt;
  double peak = 0.0;      // the solved period's aggregate, in increasing i (every lane the same sum)
  for (int i = 0; i < N; ++i) peak = peak + x0[i];
  const int jr = lane < M ? lane : (M > 0 ? M - 1 : 0);
  const bool is_row = lane < M;
  const double* cr = A.site_lds ? sre : A.cre;
  const double* ci = A.site_lds ? sim : A.cim;
  const size_t si = A.site_lds ? (size_t)M : 1, sj = A.site_lds ? 1 : (size_t)N;
  const double my_lim2 = is_row ? lim2[lane] : 0.0;

  const int bound = N * L;
  int nvis = 0;
  unsigned long long cur = 0;   // code of the visit just made; codes are ((rank << 32) | session) + 1 > 0
  for (int v = 0;; ++v) {
    // the next entry of the visiting list whose EVSE is active, cyclically behind `cur`
    unsigned long long m = kPilotsNone;
    for (int s = lane; s < Sb; s += 64) {
      const int e = sev[s];
      if ((unsigned)e >= (unsigned)N || !active[e]) continue;
      const unsigned long long code = (((unsigned long long)rank[e] << 32) | (unsigned)s) + 1;
      const unsigned long long c = code > cur ? code : code | kPilotsWrap;
      m = c < m ? c : m;
    }
    m = pilots_wave_min(m);
    if (m == kPilotsNone) break;                 // `if not active.any(): break`
    if (v == bound) { nvis = -1; break; }        // still active after N L visits: it would never end
    cur = m & ~kPilotsWrap;
    const int e = sev[(int)((cur - 1) & 0xffffffffull)];
    ++nvis;
    const double c = col[e], cp = cap[e];
    bool accept = false, retire = c >= cp;       // `if column[i] >= ub[i]: active[i] = False`
    double nxt = c;
    if (!retire) {
      // increment_in_set: the next larger level, clipped at the last finite one
      const double* le = lv + (size_t)e * L;
      double last = le[0];
      bool found = false;
      for (int k = 0; k < L; ++k) {
        const double l = le[k];
        if (l < kPilotsInf) last = l;
        if (!found && l > c && l < kPilotsInf) { nxt = l; found = true; }
      }
      if (!found) nxt = last;
      // lane j < M: re_j, im_j of the trial; lane M (and the idle ones): its aggregate.  Increasing i, one rounding per
      // product and per sum
      double re = 0.0, im = 0.0;
      for (int i = 0; i < N; ++i) {
        const double t = i == e ? nxt : col[i];
        const double a = is_row ? cr[(size_t)i * si + (size_t)jr * sj] : 1.0;
        const double bb = is_row ? ci[(size_t)i * si + (size_t)jr * sj] : 0.0;
        const double pa = a * t, pb = bb * t;
        re = re + pa;
        im = im + pb;
      }
      const double r2 = re * re, i2 = im * im;
      const bool ok = is_row ? (r2 + i2 <= my_lim2) : (re <= peak);
      accept = __all(ok ? 1 : 0) && nxt <= cp;
      retire = !accept;
    }
    if (lane == 0) {
      if (accept) col[e] = nxt;
      if (retire) active[e] = 0;
    }
    pilots_wave_sync();
  }
  for (int i = lane; i < N; i += 64) {
    const double v = col[i];
    if (fo) fo[i] = v;
    if (po) po[(size_t)i * Tm] = v;
  }
  if (lane == 0 && A.visits) A.visits[b] = nvis;
}

hipError_t launch_pilots(const PilotsArgs& a, hipStream_t st);

}  // namespace acnqp
