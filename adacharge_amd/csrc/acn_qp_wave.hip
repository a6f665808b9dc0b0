// Wave-per-problem kernel (acn_qp_wave.hpp): instantiation and launcher.
// Compiled twice, so that the two halves of the instantiations build in parallel: as it is (every EVSE k-step of
// P = Ghat r0; launch_wave, the entry) and through acn_qp_wave_e14.hip with ACNQP_WAVE_NE = 14 (the EVSE extent of the
// sites of at most 56 EVSEs; launch_wave_e14).
#include "acn_qp_launch.hpp"
#include "acn_qp_rank.hpp"
#include "acn_qp_wave.hpp"

#ifndef ACNQP_WAVE_NE
#define ACNQP_WAVE_NE 0
#endif

namespace acnqp {

static_assert(ACNQP_WAVE_NE == 0 || ACNQP_WAVE_NE == kWaveEvseExtent, "the EVSE extents instantiated: 14 k-steps and all 16");

// (which shapes come here: wave_shape, acn_qp_route.hpp; launch_wave below dispatches on the same cut points)
static_assert(kRouteWaveTS == kWaveTS, "acn_qp_route.hpp restates the period slots per lane");

// EK: the eigen extent of the instantiation (0: all k-steps, on the eigenbasis every kernel shares; otherwise the site's
// arrays in the compacted eigenbasis replace them in this launch's copy of the arguments)
// NE: the EVSE extent of P = Ghat r0 (0: all 16 k-steps), this unit's
// HIN: the launch carries host sources of lb / ub / q (TiledArgs::lb_host, the direct path for the inputs)
template <int NPW, int TSV, int MT, bool PROX, int EK, bool HIN = false, int NE = ACNQP_WAVE_NE>
static hipError_t launch_wave_prox(const TiledArgs& a_in, const WaveSite& ws, hipStream_t st) {
  TiledArgs a = a_in;
  if (EK > 0) { a.Ghat = ws.Ghat; a.lam = ws.lam; a.fragQ = ws.fragQ; }
  a.accel_mem = std::min(a.accel_mem, kWaveAM);
  const WaveLds L(a.accel_mem, NPW, MT, TSV);
  const size_t lds = (size_t)L.total * 8;
  auto kern = &admm_wave_kernel<kWaveAM, NPW, TSV, MT, PROX, EK, NE, HIN>;
  if (lds > 64 * 1024) {
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds);
    if (e != hipSuccess) return e;
  }
  // one queue position per WAVE (pair of waves): a workgroup serves kWaveNW / NPW positions at a time
  constexpr int per_wg = kWaveNW / NPW;
  const int groups = (a.B + per_wg - 1) / per_wg;
  int grid = groups;
  if (a.queue) {
    const int per_cu = resident_per_cu(reinterpret_cast<const void*>(kern), kWaveNW * 64, lds), cus = device_cus();
    const int cap = a.grid_cap > 0 ? a.grid_cap : groups;   // (a cap on WORKGROUPS: the resume launches of pipelined chunks keep theirs small)
    // A wave takes its problems one after the other, so a workgroup is as slow as the slowest of its four waves' shares:
    // only PERSISTENT workgroups level that (a workgroup per four problems wastes max-of-four against mean-of-four, 40 %).
    // The pipelined host entries (grid_oversub > 1 for the other kernels) therefore keep this kernel's grid at the resident
    // slots too; the next stream's launch moves in as this one's workgroups retire (measured, 16,384 problems per step:
    // half the chip per launch 21.4-21.8 ms, the whole chip 20.0-20.5 ms; tools/sweep_wave_pipeline.sh).
    int resident = per_cu * cus;
    static const int grid_env = std::getenv("ACNQP_WAVE_GRID") ? std::atoi(std::getenv("ACNQP_WAVE_GRID")) : 0;   // diagnostic: workgroups per pipelined launch
    if (a.grid_oversub > 1 && grid_env > 0) resident = grid_env;
    grid = std::max(1, std::min(std::min(groups, cap), resident));
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kWaveNW * 64), lds, st, a);
  return hipGetLastError();
}

// (sites without a prox row run the instantiation that carries no prox code)
template <int NPW, int TSV, int MT, int EK>
static hipError_t launch_wave_ek(const TiledArgs& a, const WaveSite& ws, hipStream_t st) {
  if (a.lb_host != nullptr) {   // (Route::direct_in: one wave per problem, and the host entry asks the route first)
    if constexpr (NPW == 1)
      return a.lf != nullptr || a.dc != nullptr ? launch_wave_prox<NPW, TSV, MT, true, EK, true>(a, ws, st) : launch_wave_prox<NPW, TSV, MT, false, EK, true>(a, ws, st);
    else
      return hipErrorInvalidValue;
  }
  return a.lf != nullptr || a.dc != nullptr ? launch_wave_prox<NPW, TSV, MT, true, EK>(a, ws, st) : launch_wave_prox<NPW, TSV, MT, false, EK>(a, ws, st);
}
// (the eigen extent: wave_eig_extent, acn_qp_rank.hpp -- a function of the site, decided once at acnqp_create)
template <int NPW, int TSV, int MT>
static hipError_t launch_wave_npw(const TiledArgs& a, const WaveSite& ws, hipStream_t st) {
  if (ws.extent == kWaveExtentSmall) return launch_wave_ek<NPW, TSV, MT, kWaveExtentSmall>(a, ws, st);
  if (ws.extent == kWaveExtentMid) return launch_wave_ek<NPW, TSV, MT, kWaveExtentMid>(a, ws, st);
  return launch_wave_ek<NPW, TSV, MT, 0>(a, ws, st);
}

template <int = 0>
static hipError_t launch_wave_shape(const TiledArgs& a, const WaveSite& ws, hipStream_t st) {
  if (a.MR == 32) return a.Tm <= kWaveTS ? launch_wave_npw<2, 6, 2>(a, ws, st) : launch_wave_npw<4, 6, 2>(a, ws, st);
  if (a.Tm > 2 * kWaveTS) return launch_wave_npw<4, 12, 1>(a, ws, st);
  return a.Tm <= kWaveTS ? launch_wave_npw<1, 12, 1>(a, ws, st) : launch_wave_npw<2, 12, 1>(a, ws, st);
}

#if ACNQP_WAVE_NE == 0
int wave_accel_columns() { return kWaveAM; }

// (the EVSE extent: wave_evse_extent, acn_qp_rank.hpp -- a function of the site's N, decided by the caller; a site it
//  does not hold never runs it)
hipError_t launch_wave(const TiledArgs& a, const WaveSite& ws, hipStream_t st) {
  if (ws.evse_ksteps == kWaveEvseExtent && a.N <= 4 * kWaveEvseExtent) return launch_wave_e14(a, ws, st);
  return launch_wave_shape(a, ws, st);
}
#else
hipError_t launch_wave_e14(const TiledArgs& a, const WaveSite& ws, hipStream_t st) { return launch_wave_shape(a, ws, st); }
#endif

}  // namespace acnqp

#if defined(ACNQP_STAMPS) && ACNQP_WAVE_NE == 0
/* diagnostic build only: the per-phase cycle counters of the wave-per-problem kernel (this unit's own g_stamps) */
extern "C" int acnqp_debug_read_wave_stamps(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(acnqp::g_stamps), sizeof(unsigned long long) * n);
}
#endif
