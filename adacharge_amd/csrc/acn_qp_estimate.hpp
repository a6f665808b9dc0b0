// The ramp-down estimator (acnqp_estimate_device / acnqp_estimate_host, include/acn_qp.h): what every EV is BELIEVED to
// accept, and the upper bounds of the next solve capped with it.  Between the advance and the prepare entry of a closed
// loop: the reference's estimate_max_rate (ada.py:143-146) with acnportal's SimpleRampdown.  An EV in the tail of a
// two-stage battery draws less than it is offered; the estimate follows what it drew, so the solver stops reserving
// infrastructure capacity for current the EV will not take, and probes upwards again when the EV draws all it may.
// K = 1: online MPC, one session per EVSE.  Units are the slot state's: amperes.
//
// tests/estimate_spec.py states the six rules of include/acn_qp.h in plain loops; the kernel is held to it BIT FOR BIT.
// Everything is a copy or a comparison except at most two subtractions and one addition per EVSE, each rounded once.
//
// One workgroup per problem, its size chosen by the shape only (prepare_threads' rule): ONE wavefront for N <= 64, four
// beyond.  Phase 1: one thread per EVSE (in a loop beyond THREADS) applies rules 1-4, stores est' and leaves the bound u
// and the window length in LDS (12 bytes per EVSE).  Phase 2, after one barrier: all threads stream the N * Tm elements of
// lb, ub -> ub_out, coalesced over k = i * Tm + t as the advance's shift does.  The flags: __any inside a wavefront; across
// the four, every wavefront stores its two bits into its own BYTE of one LDS word and thread 0 reads the word after the
// barrier.  No atomics; every output element is written whatever the input; a problem gives the same bits alone and at
// any position of any batch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace acnqp {

constexpr int kEstimateBadFresh = 1;   // bits of flags[b] (ACNQP_ESTIMATE_* of include/acn_qp.h)
constexpr int kEstimateBadSlot = 2;

struct EstimateArgs {
  int B, N, Tm;
  const int32_t *s_off, *s_len;   // [B][N]
  const double *lb, *ub;          // [B][N][Tm]
  const int32_t* fresh;           // [B][N]
  const double* pilots;           // [B][N] or nullptr: no history
  const double* actual;           // [B][N] or nullptr: what is offered is drawn
  const int32_t* status;          // [B] or nullptr
  double up_threshold, down_threshold, up_increment;
  double* est;                    // [B][N] in and out
  double* ub_out;                 // [B][N][Tm]
  int32_t* flags;                 // [B]
};

inline int estimate_threads(int N) { return N <= 64 ? 64 : 256; }   // (prepare_threads' rule)
inline size_t estimate_lds_bytes(int N) { return (size_t)N * 12; }  // u [N] doubles, then the window lengths [N]

template <int THREADS>
__global__ __launch_bounds__(THREADS) void estimate_kernel(const EstimateArgs A) {
#pragma clang fp contract(off)   // the subtractions and the addition of this kernel are rounded once each (tests/estimate_spec.py)
  extern __shared__ __attribute__((aligned(16))) char estimate_lds[];
  __shared__ uint32_t wave_bits;   // byte w: the flag bits of wavefront w (THREADS == 256 only)
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int N = A.N, Tm = A.Tm;
  double* s_u = reinterpret_cast<double*>(estimate_lds);   // the bound of EVSE i
  int* s_n = reinterpret_cast<int*>(s_u + N);              // its window length; 0: no cap
  const size_t sb = (size_t)b * N, pb = sb * Tm;
  bool served = true;
  if (A.status) {
    const int s = A.status[b];
    served = s == 1 || s == 5;   // ACNQP_STATUS_SOLVED, _SOLVED_INACCURATE: the advance's rule 1
  }
  // ---- phase 1: rules 1-4, one thread per EVSE ------------------------------------------------------------------------
  int bad = 0;
  for (int i = gt; i < N; i += THREADS) {
    const size_t e = sb + i;
    // 1 slot
    const int ln = A.s_len[e];
    const bool fr = A.fresh[e] != 0;
    if (ln > Tm) bad |= kEstimateBadSlot;
    const bool present = ln > 0 && A.s_off[e] == 0 && ln <= Tm;
    double u = __builtin_huge_val();
    if (!present) {
      // 2 absent
      if (fr) bad |= kEstimateBadFresh;
    } else if (fr) {
      // 3 first sight
      u = A.ub[pb + (size_t)i * Tm];
    } else {
      // 4 update
      u = A.est[e];
      if (A.pilots) {
        const double pi = A.pilots[e];
        const double pp = served && pi > 0.0 ? pi : 0.0;
        double pr = pp;
        if (A.actual) pr = served ? A.actual[e] : 0.0;
        if (pp - pr > A.down_threshold) {
          u = pr + A.up_increment;
        } else if (u - pr < A.up_threshold) {
          u = u + A.up_increment;
        }
      }
    }
    // 5 output: est' here, the bounds in phase 2
    A.est[e] = u;
    s_u[i] = u;
    s_n[i] = present ? ln : 0;
  }
  // 6 flags
  const int fresh_bit = __any(bad & kEstimateBadFresh) ? kEstimateBadFresh : 0;
  const int slot_bit = __any(bad & kEstimateBadSlot) ? kEstimateBadSlot : 0;
  if constexpr (THREADS != 64) {
    if ((gt & 63) == 0) reinterpret_cast<uint8_t*>(&wave_bits)[gt >> 6] = (uint8_t)(fresh_bit | slot_bit);
  }
  __syncthreads();
  if (gt == 0) {
    if constexpr (THREADS == 64) {
      A.flags[b] = fresh_bit | slot_bit;
    } else {
      const uint32_t w = wave_bits;
      A.flags[b] = (int)((w | (w >> 8) | (w >> 16) | (w >> 24)) & 3u);
    }
  }
  // ---- phase 2: rule 5, the capped bounds, streamed by all threads ------------------------------------------------------
  const double *lb = A.lb + pb, *ub = A.ub + pb;
  double* out = A.ub_out + pb;
  const int n = N * Tm;
  for (int k = gt; k < n; k += THREADS) {
    const int i = k / Tm, t = k - i * Tm;
    double v = ub[k];
    const double lo = lb[k];
    if (t < s_n[i]) {
      const double u = s_u[i];
      v = u < v ? u : v;
      v = v < lo ? lo : v;
    }
    out[k] = v;
  }
}

hipError_t launch_estimate(const EstimateArgs& a, hipStream_t st);

}  // namespace acnqp
