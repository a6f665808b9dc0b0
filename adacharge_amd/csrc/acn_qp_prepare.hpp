// Before the solve (acnqp_prepare_device / acnqp_prepare_host, include/acn_qp.h): the link between the advance kernel's slot
// state and the two steps of the reference that read the SESSION LIST -- apply_minimum_charging_rate (ada.py:147-150), a
// greedy walk over the sessions in arrival order, and diff_based_reallocation (post.py:214-218), whose round robin breaks
// ties of the rounding loss by list order.  The slot state carries no order; the caller states it as one int32 key per
// EVSE and problem (the session's position in its list), and this kernel turns state plus keys into
//   (a) the first-period bounds the reference's pre-processing would have produced (rule 2), and
//   (b) the session arrays acnqp_pilot_plan wants, in list order (rule 3).
// K = 1: online MPC, one session per EVSE.
//
// tests/prepare_spec.py states the four rules of include/acn_qp.h in plain loops; the kernel is held to it BIT FOR BIT.
// Everything is a copy or a comparison except the row test of the walk: the arithmetic of the pilots kernel's row test
// (increasing i inside ONE lane, every product and sum rounded once, squares compared) in a copy of its own -- calling one
// shared function from both kernels cost the pilots kernel a register (57 -> 58 VGPRs), see DESIGN.md section 3.6e.
//
// One workgroup per problem, its size chosen by the shape only (prepare_threads): ONE wavefront for N <= 64, four beyond.
//   1  keys, caps, period-0 bounds, min pilots and -- where they fit (prepare_layout, shape only) -- the site rows into LDS
//   2  one thread per EVSE: its position in the view = the count of smaller (key, i) pairs among the live slots, or, for an
//      EVSE without a live slot, the live count plus the dead EVSEs before it; ord[position] = EVSE (a permutation of
//      0 .. N-1: nothing has a capacity)
//   3  the first wavefront walks ord alone (wavefront-scope fences, no workgroup barrier inside the walk): at most N visits,
//      row j's sums in lane j (rows beyond the wavefront in a loop), w broadcast from LDS
//   4  all threads write period 0 of the present slots, the view and the flag
// No atomics; every view element and every flag is written whatever the input; a problem gives the same bits alone and at
// any position of any batch.
#pragma once
#include "acn_qp_pilots.hpp"

namespace acnqp {

constexpr int kPrepareFuture = 1;   // bit of flags[b]: a live slot with s_off > 0

struct PrepareArgs {
  int B, N, Tm, M;
  const int32_t *s_off, *s_len;   // [B][N]
  const double* s_cap;            // [B][N]
  double *lb, *ub;                // [B][N][Tm]: period 0 is read, and written under min_pilot
  const int32_t* key;             // [B][N] read where the slot is live
  const double *cre, *cim;        // [M][N]
  const double* limits;           // [M]
  const double* min_pilot;        // [N] or nullptr: no rule 2
  int32_t* v_evse;                // [B*N] or nullptr (the three together)
  uint8_t* v_arrived;
  double* v_cap;
  int32_t* flags;                 // [B]
  int site_lds;                   // prepare_layout
};

struct PrepareLayout {
  int site_lds;
  size_t bytes;
};
inline PrepareLayout prepare_layout(int N, int M) {
  PrepareLayout p{0, 0};
  const size_t budget = 60 * 1024;
  size_t need = (size_t)N * (5 * 8 + 3 * 4) + (size_t)(M + 2) * 8;
  const size_t site = (size_t)2 * M * N * 8;
  if (M > 0 && need + site <= budget) { p.site_lds = 1; need += site; }
  p.bytes = (need + 15) & ~(size_t)15;
  return p;
}
inline int prepare_threads(int N) { return N <= 64 ? 64 : 256; }

// re_j, im_j of one site row (coefficients at i * si + row) over the column t with t[e] replaced by `trial`: increasing i,
// one rounding per product and per sum -- the loop of pilots_kernel's acceptance test without its aggregate lane
struct PrepareSums { double re, im; };
__device__ inline PrepareSums prepare_row_sums(const double* t, int N, int e, double trial, const double* cr, const double* ci, size_t si,
                                               size_t row) {
#pragma clang fp contract(off)
  double re = 0.0, im = 0.0;
  for (int i = 0; i < N; ++i) {
    const double v = i == e ? trial : t[i];
    const double pa = cr[(size_t)i * si + row] * v, pb = ci[(size_t)i * si + row] * v;
    re = re + pa;
    im = im + pb;
  }
  return {re, im};
}
// re^2 + im^2 <= (limit + 1e-7)^2: squares, no sqrt, no hypot
__device__ inline bool prepare_row_ok(double re, double im, double lim2) {
#pragma clang fp contract(off)
  const double r2 = re * re, i2 = im * im;
  return r2 + i2 <= lim2;
}

constexpr int kPrepLive = 1, kPrepPresent = 2, kPrepFuture = 4;   // bits of the staged slot state

template <int THREADS>
__global__ __launch_bounds__(THREADS) void prepare_kernel(const PrepareArgs A) {
#pragma clang fp contract(off)   // every product and every sum of this kernel is rounded once (tests/prepare_spec.py)
  extern __shared__ __attribute__((aligned(16))) char prepare_lds[];
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int N = A.N, Tm = A.Tm, M = A.M;
  const size_t sb = (size_t)b * N;
  double* lb = A.lb + sb * Tm;
  double* ub = A.ub + sb * Tm;
  const bool walk = A.min_pilot != nullptr;

  // ---- LDS carve (prepare_layout) -----------------------------------------------------------------------------------
  double* cap = reinterpret_cast<double*>(prepare_lds);   // [N]
  double* lb0 = cap + N;                                  // [N] period 0 of the bounds
  double* ub0 = lb0 + N;
  double* w = ub0 + N;                                    // [N] the minimum rates granted so far
  double* mp = w + N;                                     // [N] min_pilot
  double* lim2 = mp + N;                                  // [M + 2]: (limit + 1e-7)^2 per row
  double* sre = lim2 + M + 2;                             // [N][M] site rows, EVSE-major (lane = row reads neighbours)
  double* sim = sre + (A.site_lds ? (size_t)M * N : 0);
  int* key = reinterpret_cast<int*>(sim + (A.site_lds ? (size_t)M * N : 0));   // [N]
  int* st = key + N;                                      // [N] kPrepLive | kPrepPresent | kPrepFuture
  int* ord = st + N;                                      // [N] EVSE at each position of the view

  // ---- 1: stage ---------------------------------------------------------------------------------------------------------
  for (int i = gt; i < N; i += THREADS) {
    const int off = A.s_off[sb + i], len = A.s_len[sb + i];
    const bool live = len > 0;
    st[i] = (live ? kPrepLive : 0) | (live && off == 0 ? kPrepPresent : 0) | (live && off > 0 ? kPrepFuture : 0);
    key[i] = live ? A.key[sb + i] : 0;
    cap[i] = A.s_cap[sb + i];
    lb0[i] = lb[(size_t)i * Tm];
    ub0[i] = ub[(size_t)i * Tm];
    w[i] = 0.0;
    mp[i] = walk ? A.min_pilot[i] : 0.0;
  }
  if (walk) {
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
  }
  __syncthreads();

  // ---- 2: rule 1, the position of every EVSE in the view (comparisons only) ----------------------------------------------
  for (int i = gt; i < N; i += THREADS) {
    const bool li = (st[i] & kPrepLive) != 0;
    const int ki = key[i];
    int smaller = 0, nlive = 0, dead_before = 0;
    for (int k = 0; k < N; ++k) {
      const bool lk = (st[k] & kPrepLive) != 0;
      const int kk = key[k];
      nlive += lk ? 1 : 0;
      smaller += lk && (kk < ki || (kk == ki && k < i)) ? 1 : 0;
      dead_before += !lk && k < i ? 1 : 0;
    }
    ord[li ? smaller : nlive + dead_before] = i;   // a permutation: the positions are distinct and below N
  }
  __syncthreads();

  // ---- 3: rule 2, the greedy walk: sequential, the first wavefront runs it alone ---------------------------------------------
  if (walk && gt < 64) {
    const int lane = gt;
    const double* cr = A.site_lds ? sre : A.cre;
    const double* ci = A.site_lds ? sim : A.cim;
    const size_t si = A.site_lds ? (size_t)M : 1, sj = A.site_lds ? 1 : (size_t)N;
    for (int r = 0; r < N; ++r) {
      const int e = ord[r];
      if (!(st[e] & kPrepPresent)) continue;   // (uniform: every lane reads the same word)
      const double want = mp[e];
      bool ok = true;
      for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        const bool is_row = j < M;
        const int jr = is_row ? j : M - 1;
        const PrepareSums sm = prepare_row_sums(w, N, e, want, cr, ci, si, (size_t)jr * sj);   // (an idle lane repeats the last row)
        ok = ok && (!is_row || prepare_row_ok(sm.re, sm.im, lim2[jr]));
      }
      const bool accept = __all(ok ? 1 : 0) && cap[e] >= want;
      if (lane == 0) {
        if (accept) {
          const double l0 = lb0[e], l = l0 > want ? l0 : want;
          const double u = ub0[e];
          w[e] = want;
          lb0[e] = l;
          ub0[e] = u < l ? l : u;
        } else {
          lb0[e] = 0.0;
          ub0[e] = 0.0;
        }
      }
      pilots_wave_sync();
    }
  }
  __syncthreads();

  // ---- 4: period 0 of the present slots, rule 3 (the view), rule 4 (the flag) ---------------------------------------------
  if (walk)
    for (int i = gt; i < N; i += THREADS)
      if (st[i] & kPrepPresent) {
        lb[(size_t)i * Tm] = lb0[i];
        ub[(size_t)i * Tm] = ub0[i];
      }
  if (A.v_evse)
    for (int r = gt; r < N; r += THREADS) {
      const int i = ord[r];
      const bool here = (st[i] & kPrepPresent) != 0;
      const double c = cap[i], u = ub0[i];
      A.v_evse[sb + r] = i;
      A.v_arrived[sb + r] = here ? 1 : 0;
      A.v_cap[sb + r] = here ? (c <= u ? c : u) : 0.0;
    }
  if (gt < 64) {
    int bad = 0;
    for (int i = gt; i < N; i += 64) bad |= st[i] & kPrepFuture;
    const bool any = __any(bad);
    if (gt == 0) A.flags[b] = any ? kPrepareFuture : 0;
  }
}

hipError_t launch_prepare(const PrepareArgs& a, hipStream_t st);

}  // namespace acnqp
