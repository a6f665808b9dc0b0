// The plant (acnqp_plant_device / acnqp_plant_host, include/acn_qp.h): what every EV DRAWS of the pilot it is offered.  Between
// the pilots entry and the advance of a closed loop: the advance's rule 1 takes `applied` as delivered, and without this
// kernel the loop hands it the pilots themselves -- an EV that draws exactly what it is offered.  Here a battery per EV
// decides: a current limit, the room left to full, and in the two-stage model a tail in which the rate it accepts falls in
// proportion to that room (acnportal's Battery and Linear2StageBattery in their stepwise form).
// K = 1: online MPC, one session per EVSE.  Units are the slot state's: amperes and ampere-periods.
//
// tests/plant_spec.py states the five rules of include/acn_qp.h in plain loops; the kernel is held to it BIT FOR BIT.
// Everything is a copy or a comparison except one product (the tail's rate) and one subtraction (the room), each rounded
// once; there is no division -- the caller's table carries the tail's slope.
//
// One workgroup per problem, its size chosen by the shape only (prepare_threads' rule): ONE wavefront for N <= 64, four
// beyond.  One thread per EVSE, in a loop beyond THREADS.  The flag: __any inside a wavefront; across the four, every
// wavefront stores its two bits into its own BYTE of one LDS word and thread 0 reads the word after a barrier.
// No atomics; every output element is written whatever the input; a problem gives the same bits alone and at any position
// of any batch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace acnqp {

constexpr int kPlantBadPlug = 1;      // bits of flags[b] (ACNQP_PLANT_* of include/acn_qp.h)
constexpr int kPlantBadBattery = 2;

struct PlantArgs {
  int B, N, R;                                      // problems, EVSEs, rows of the battery table
  const int32_t *s_off, *s_len;                     // [B][N]
  const double* pilots;                             // [B][N]
  const int32_t* status;                            // [B] or nullptr
  const double *t_room, *t_amps, *t_knee, *t_slope; // [R]
  const int32_t* plug;                              // [B][N] the row plugged in now, or < 0
  int32_t* bat;                                     // [B][N] in and out
  double* room;                                     // [B][N] in and out
  double* actual;                                   // [B][N]
  int32_t* flags;                                   // [B]
};

inline int plant_threads(int N) { return N <= 64 ? 64 : 256; }   // (prepare_threads' rule)

template <int THREADS>
__global__ __launch_bounds__(THREADS) void plant_kernel(const PlantArgs A) {
#pragma clang fp contract(off)   // the product and the subtraction of this kernel are rounded once each (tests/plant_spec.py)
  __shared__ uint32_t wave_bits;   // byte w: the flag bits of wavefront w (THREADS == 256 only)
  const int gt = (int)threadIdx.x, b = (int)blockIdx.x;
  const int N = A.N, R = A.R;
  const size_t sb = (size_t)b * N;
  bool served = true;
  if (A.status) {
    const int s = A.status[b];
    served = s == 1 || s == 5;   // ACNQP_STATUS_SOLVED, _SOLVED_INACCURATE: the advance's rule 1
  }
  int bad = 0;
  for (int i = gt; i < N; i += THREADS) {
    const size_t e = sb + i;
    int r = A.bat[e];
    double rm = A.room[e];
    // 1 plug
    const int pl = A.plug[e];
    if (pl >= R) {
      bad |= kPlantBadPlug;
    } else if (pl >= 0) {
      r = pl;
      rm = A.t_room[pl];
    }
    // 2 offer
    const bool present = A.s_len[e] > 0 && A.s_off[e] == 0;
    const double pi = A.pilots[e];
    const double p = present && served && pi > 0.0 ? pi : 0.0;
    // 3 draw
    double a = p;
    if (r >= R) {
      bad |= kPlantBadBattery;
    } else if (r >= 0) {
      double lim = A.t_amps[r];
      const double knee = A.t_knee[r];
      if (knee > 0.0 && rm <= knee) {
        const double v = rm * A.t_slope[r];
        lim = v < lim ? v : lim;
      }
      a = lim < a ? lim : a;
      a = rm < a ? rm : a;
      a = a < 0.0 ? 0.0 : a;
      rm = rm - a;
    }
    // 4 output
    A.actual[e] = a;
    A.bat[e] = r;
    A.room[e] = rm;
  }
  // 5 flags
  const int plug_bit = __any(bad & kPlantBadPlug) ? kPlantBadPlug : 0;
  const int bat_bit = __any(bad & kPlantBadBattery) ? kPlantBadBattery : 0;
  if constexpr (THREADS == 64) {
    if (gt == 0) A.flags[b] = plug_bit | bat_bit;
  } else {
    if ((gt & 63) == 0) reinterpret_cast<uint8_t*>(&wave_bits)[gt >> 6] = (uint8_t)(plug_bit | bat_bit);
    __syncthreads();
    if (gt == 0) {
      const uint32_t w = wave_bits;
      A.flags[b] = (int)((w | (w >> 8) | (w >> 16) | (w >> 24)) & 3u);
    }
  }
}

hipError_t launch_plant(const PlantArgs& a, hipStream_t st);

}  // namespace acnqp
