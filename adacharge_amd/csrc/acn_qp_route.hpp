// The routing table: every decision the host takes from a problem's SHAPE, written once -- the padded row count of a
// site, the kernel family of a launch, and what follows from the family (workspace per workgroup, Anderson-column cap,
// wanted chunk size, polish eligibility).  Host code only: no HIP, no handle, no getenv (the diagnostic switches come in
// as a struct), so tests/test_route_table.py compiles this header with the host compiler and pins every cut point
// without a GPU.  acn_qp_api.hip asks this table and nothing else; acnqp_route reports what it says.
#pragma once
#include <algorithm>

#include "acn_qp.h"

namespace acnqp {

constexpr int kRouteMaxK = 4;     // session slots per EVSE of the on-chip kernels (== kMaxK, asserted in acn_qp_api.hip)
constexpr int kRouteWaveTS = 12;  // period slots per lane of the wave kernel (== kWaveTS, asserted in acn_qp_wave.hip)

// ---- site shape -------------------------------------------------------------------------------------------------------
// Site rows in the kernels' internal order, before rounding up to whole 16-row tiles: SOC pads its 2 M rows to
// 8 * ceil(M / 4) (pairs sit in adjacent registers of one lane, acn_qp_tiled.hpp), then one row per peak / flat / max.
// acnqp_create refuses a site with more than 48.
inline int padded_rows(int cone, int M, int has_peak, int has_flat, int has_max) {
  return (cone == ACNQP_CONE_SOC ? 8 * ((M + 3) / 4) : M) + (has_peak ? 1 : 0) + (has_flat ? 1 : 0) + (has_max ? 1 : 0);
}

struct SiteShape {
  int N = 0, M = 0, Mg = 0, MR = 0;   // EVSEs, infrastructure constraints, rows at the ABI, padded rows (multiple of 16, >= 16)
  int cone = 0, has_peak = 0, has_flat = 0, has_max = 0;
  int NP() const { return N <= 64 ? 64 : 16 * ((N + 15) / 16); }   // padded EVSEs
};

inline SiteShape site_shape(int N, int M, int cone, int has_peak, int has_flat, int has_max) {
  SiteShape s;
  s.N = N; s.M = M; s.cone = cone;
  s.has_peak = has_peak ? 1 : 0; s.has_flat = has_flat ? 1 : 0; s.has_max = has_max ? 1 : 0;
  s.Mg = (cone == ACNQP_CONE_SOC ? 2 * M : M) + s.has_peak + s.has_flat + s.has_max;
  s.MR = 16 * std::max(1, (padded_rows(cone, M, has_peak, has_flat, has_max) + 15) / 16);
  return s;
}

// ---- diagnostic switches (environment variables of the same names with ACNQP_ in front; acn_qp_api.hip reads them) -----
struct RouteSwitches {
  bool no_wave = false;     // NO_WAVE: the register-resident tiled kernel instead of the wave kernel
  bool no_wave2 = false;    // NO_WAVE2: ... for every variant but the first
  int wave_min_batch = 1;   // WAVE_MIN_BATCH: launches of fewer problems do not take the wave kernel
  bool no_long = false;     // NO_LONG: the general-shape kernel instead of the long-horizon kernel
  bool lds_long = true;     // LDS_LONG=0: the long-horizon kernel's workspace variant instead of its LDS-resident one
};

// ---- predicates ---------------------------------------------------------------------------------------------------------
// Shapes the wave-per-problem kernel takes: a lane per EVSE, twelve period registers, one session slot, box / disc / peak
// rows and the two prox rows.  A function of the SHAPE only, never of the batch size: a problem's result does not depend
// on what it is batched with (tests/test_gpu_parity.py asserts the bits); `batch` enters only through the diagnostic
// wave_min_batch.  The price: a problem is ONE wave's dependent chain here (4.3 us per iteration) and four waves' in the
// tiled kernel (3.1 us alone on a CU), so a launch of at most one problem per CU ends later than it did (256 problems:
// 2.9 against 2.3 ms; one problem: 0.85 against 0.6 ms) -- from two problems per CU on, four problems in flight per CU
// win (16,384: 26.5 -> 15.5 ms).  Returns the variant (0: not this kernel; 1: horizon <= 12, one wave per problem;
// 2: horizon 13 ... 24, two waves; 3: two row tiles at horizon <= 12, two waves of six periods; 4: two row tiles at
// horizon 13 ... 24, four waves of six periods -- one problem per workgroup; 5: one row tile at horizon 33 ... 48, four
// waves of twelve periods).  (A demand-charge row does not matter: its prox couples all periods, and its sums cross the
// group's mailbox.)
inline int wave_shape(const SiteShape& s, int t_max, int k_sessions, int batch, const RouteSwitches& sw) {
  constexpr int TS = kRouteWaveTS;
  const bool off2 = sw.no_wave2;
  if (sw.no_wave || s.N > 64 || k_sessions != 1 || batch < sw.wave_min_batch) return 0;
  if (s.MR == 16 && t_max <= TS) return 1;                   // one wave per problem
  if (s.MR == 16 && t_max <= 2 * TS) return off2 ? 0 : 2;    // two waves, twelve periods each
  // (horizons 25 ... 32 stay with the tiled kernel's two column tiles: the same four waves per problem there, 19.8 against
  //  21.3 ms at 2,048 problems; from 33 on the alternative streams its state: 57.0 against 22.3 ms at horizon 48)
  if (s.MR == 16 && t_max > 32 && t_max <= 4 * TS) return off2 ? 0 : 5;   // horizon 33 ... 48: four waves, twelve periods each
  if (s.MR == 32 && t_max <= TS) return off2 ? 0 : 3;        // two row tiles: two waves, six periods each
  if (s.MR == 32 && t_max <= 2 * TS) return off2 ? 0 : 4;    // two row tiles, horizon 13 ... 24: four waves, six periods each
  return 0;
}

// Shapes the register-resident tiled kernel takes: N <= 64, one column tile with any number of row tiles, or two
// column tiles with ONE row tile.  Two column tiles x two / three row tiles (horizon 17 ... 32 on a site of more than 16
// padded rows, e.g. the synthetic JPL site at horizon 24 of configs[2]) are not register-resident -- every wave would
// carry the whole site-row state redundantly (430-1,100 spilled registers; those instantiations are gone): two row
// tiles run through the LDS-resident variant of the long-horizon kernel (measured on 4,096 jpl52 x 24 problems: 189 ms
// tiled, 70 ms there), or its workspace variant with a demand-charge row / lds_long off (diagnostic); three row
// tiles through the general-shape kernel.
inline bool tiled_shape(const SiteShape& s, int t_max, int k_sessions) {
  if (t_max > 16 && s.MR > 16) return false;   // two column tiles x two / three row tiles: not register-resident
  return s.N <= 64 && t_max <= 32 && k_sessions <= kRouteMaxK;
}
inline bool lds_long_shape(const SiteShape& s, int t_max, const RouteSwitches& sw) {
  return sw.lds_long && s.N <= 64 && t_max > 16 && t_max <= 32 && !s.has_max && s.MR == 32;
}
// shapes the large-site MFMA kernel takes (acn_qp_stream.hpp): wide sites, up to three column tiles
inline bool stream_shape(const SiteShape& s, int t_max) { return s.N > 64 && t_max <= 48; }
// shapes the long-horizon MFMA kernel takes (acn_qp_long.hpp): what the two kernels above leave, up to 288 periods and
// two row tiles.  (A wave-5 shape -- one row tile, horizon 33 ... 48 -- is one of these too; route_for asks the wave
// kernel first.)
inline bool long_shape(const SiteShape& s, int t_max, int k_sessions, const RouteSwitches& sw) {
  return !sw.no_long && !tiled_shape(s, t_max, k_sessions) && !stream_shape(s, t_max) && t_max <= 288 && s.MR <= 32;
}

// ---- the route of one launch ---------------------------------------------------------------------------------------------
struct Route {
  int family = 0;     // ACNQP_ROUTE_*
  int wv = 0;         // wave-per-problem variant (0: another family)
  bool tiled = false, stream = false, lng = false, lds = false, on_chip = false;
  bool polish_shape = false;   // the shape's half of the polish decision (the LDS fit and the options: acn_qp_api.hip)
  bool polish_long_shape = false;   // the shape's half of the LONG-horizon polish decision (acn_qp_polish_long.hpp; the handle's
                                    // switch acnqp_set_long_polish and the options: acn_qp_api.hip).  Never true with polish_shape.
  bool polish_wide_shape = false;   // the shape's half of the WIDE-site polish decision (acn_qp_polish_wide.hpp; the handle's switch
                                    // acnqp_set_wide_polish and the options: acn_qp_api.hip).  Never true with the other two.
  SiteShape site;     // what it was decided for
  int t_max = 0, k_sessions = 0;

  // Problems per chunk the host pipeline wants for this shape: large enough that the launch tail (its slowest problems)
  // is short.  The register-resident kernel takes 1,024 (two per workgroup slot): with the launches sorted longest-first
  // and four streams in flight the shorter pipeline head and tail outweigh the per-launch tails (bench: 441 -> 455 k
  // QP/s).  The wave kernel's launches are persistent (four problems in flight per CU, one wave each): a launch ends
  // with its slowest problem whatever its size, so few large chunks (sweep at 16,384 problems per call: 4,096 / 6,144 /
  // 7,168 / 8,192 / 9,216 -> 18.9 / 19.0 / 18.3 / 18.0 / 19.4 ms).  As measured, not as named: the 1,024 belong to
  // tiled_shape, so the LDS-resident long-horizon family takes 2,048 although it is on_chip, and wave variant 5 takes
  // 8,192 although tiled_shape is false for it.
  long long chunk_want() const { return wv > 0 ? 8192 : (tiled ? 1024 : 2048); }

  // The kernel can store a problem's schedule straight into a device-addressable host array (TiledArgs::x_host; the host
  // entries then copy no x back and plan their chunks without the small last one, acn_qp_pipeline.hpp): the wave kernel
  // with one wave per problem.  By shape alone.
  bool direct_x() const { return wv == 1; }

  // The kernel can load a problem's lb / ub / q straight from device-addressable host arrays (TiledArgs::lb_host ...; the
  // dense host entry then copies none of the three for the call's leading chunk, acn_qp_pipeline.hpp): the wave kernel
  // with one wave per problem, and nothing else.  By shape alone.
  bool direct_in() const { return wv == 1; }

  // Anderson columns the family can hold (acnqp_accel_columns = min(requested, this)); `Kn`: the kernels' own numbers
  template <class Kn> int accel_cap() const {
    if (wv > 0) return Kn::wave_accel();
    if (tiled) return Kn::tiled_accel(site.MR / 16, (t_max + 15) / 16, site.NP(), k_sessions);
    if (stream) return Kn::stream_accel();
    if (lng) return Kn::long_accel();
    return Kn::general_accel();
  }

  // doubles of workspace one workgroup of the family needs with `accel_req` columns requested (0: state on chip)
  template <class Kn> long long workspace_doubles(int accel_req) const {
    if (tiled) return 0;
    const int accel = std::min(std::max(0, accel_req), accel_cap<Kn>());
    if (stream) return Kn::stream_workspace(site.NP(), (t_max + 15) / 16, k_sessions, site.MR / 16, accel);
    if (lng) return Kn::long_workspace(site.NP(), t_max, k_sessions, site.MR / 16, accel);
    const long long n = (long long)site.N * t_max, mt = (long long)site.MR * t_max, Dn = n + mt;
    // general-shape kernel: solver state, the certificate's dual snapshot, the Anderson vectors (u, f: reals; correction
    // and rings: floats)
    return 7 * n + 8 * mt + 3LL * k_sessions * site.N + 8 + 2 * Dn + ((1 + 2LL * accel) * Dn * 4 + 7) / 8 + 2;
  }
};

// The kernel family a launch of this shape runs: the ONE place the choice is made (the launch and acnqp_route both ask it,
// so that what the tests query is what runs).
inline Route route_for(const SiteShape& s, int t_max, int k_sessions, int batch, const RouteSwitches& sw) {
  Route r;
  r.site = s; r.t_max = t_max; r.k_sessions = k_sessions;
  r.wv = wave_shape(s, t_max, k_sessions, batch, sw);
  r.tiled = r.wv > 0 || tiled_shape(s, t_max, k_sessions);   // (no workspace: state on chip)
  r.stream = !r.tiled && stream_shape(s, t_max);
  r.lng = !r.tiled && long_shape(s, t_max, k_sessions, sw);
  r.lds = r.lng && lds_long_shape(s, t_max, sw);
  r.on_chip = r.tiled || r.lds;
  if (r.wv > 0) r.family = r.wv;   // ACNQP_ROUTE_WAVE1 ... ACNQP_ROUTE_WAVE5
  else if (r.tiled) r.family = t_max <= 16 ? ACNQP_ROUTE_TILED_CT1 : ACNQP_ROUTE_TILED_CT2;
  else if (r.stream) r.family = ACNQP_ROUTE_STREAM;
  else if (r.lng) r.family = r.lds ? ACNQP_ROUTE_LONG_LDS : ACNQP_ROUTE_LONG_WS;
  else r.family = ACNQP_ROUTE_GENERAL;
  // the polish (acn_qp_polish.hpp): small sites, separable objective, served by an on-chip kernel
  r.polish_shape = r.on_chip && s.N <= 64 && t_max <= 32 && k_sessions <= kRouteMaxK && !s.has_flat && !s.has_max &&
                   s.M + s.has_peak > 0;
  // the long-horizon polish (acn_qp_polish_long.hpp): the same sites at horizons 33 ... 288, behind the four-wave route and
  // the long-horizon kernel's workspace variant (not the general kernel's three row tiles)
  r.polish_long_shape = s.N <= 64 && t_max > 32 && t_max <= 288 && k_sessions <= kRouteMaxK && !s.has_flat && !s.has_max &&
                        s.M + s.has_peak > 0 && (r.family == ACNQP_ROUTE_WAVE5 || r.family == ACNQP_ROUTE_LONG_WS);
  // the wide-site polish (acn_qp_polish_wide.hpp): behind the large-site kernel's launch, sites of up to 1,024 EVSEs whose
  // session slots make at most 1,024 columns (8 ceil(N K / 8): the capacitance matrix's tables) and whose site has at most
  // 48 rows at the ABI
  r.polish_wide_shape = r.family == ACNQP_ROUTE_STREAM && s.N > 64 && s.N <= 1024 && t_max <= 48 && k_sessions <= kRouteMaxK &&
                        8 * ((s.N * k_sessions + 7) / 8) <= 1024 && s.Mg <= 48 && !s.has_flat && !s.has_max && s.M + s.has_peak > 0;
  return r;
}

// (acnqp_accel_columns asks as if the batch were unbounded: wave_min_batch never lowers its answer)
constexpr int kRouteAnyBatch = 1 << 30;

}  // namespace acnqp
