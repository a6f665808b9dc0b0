// The polish plan: everything the host decides about the Newton polish of ONE launch, written once -- whether the launch
// is polished and by which kernel (on-chip acn_qp_polish.hpp, long-horizon acn_qp_polish_long.hpp, wide-site
// acn_qp_polish_wide.hpp), the sizes of that kernel's tables, how the launch's scratch buffer is carved up, and the
// polish launch's grid.  Host code only, in the manner of acn_qp_route.hpp: no HIP, no handle, no getenv (the switches come
// in as a struct), so tests/test_polish_plan.py compiles this header with the host compiler and pins it without a GPU.
// acn_qp_api.hip asks this plan and nothing else; acnqp_route reports what it says for the default options.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "acn_qp_route.hpp"
#include "acn_qp_pollds.hpp"
#include "acn_qp_polslab.hpp"
#include "acn_qp_polwide.hpp"

namespace acnqp {

enum class PolishKind { none, on_chip, long_horizon, wide };

// what is not the shape's or the options': ACNQP_NO_POLISH (diagnostic) and the handle's two switches (acn_qp_api.hip fills it)
struct PolishSwitches {
  bool no_polish = false;     // NO_POLISH: no launch is polished
  bool long_polish = false;   // acnqp_set_long_polish
  bool wide_polish = false;   // acnqp_set_wide_polish
};

struct PolishPlan {
  PolishKind kind = PolishKind::none;
  int max_rows = 0;          // PolishArgs::max_rows: rows of the Schur system the row tables hold
  int max_sess = 0;          // PolishArgs::max_sess: session columns the capacitance matrix holds
  int blk_doubles = 0;       // PolishArgs::blk_doubles: doubles of the packed per-period blocks
  int rows_for_solver = 0;   // TiledArgs::pol_rows: the row count beyond which the solver declines a hand-over (polish_fits asks
                             // for 8 rows of head room: the long kernel's tables hold the worst case, so it never declines)
};

// The plan of a launch of route `rt` under the options' polish_iters and max_iter; `warm`: the caller gives warm_x and
// warm_y.  By shape, switches and options, never by the batch size: a problem's result must not depend on what it is
// batched with (tests/test_batch_invariance.py).  The route's three shape flags never overlap.
inline PolishPlan polish_plan(const Route& rt, const PolishSwitches& sw, int polish_iters, int max_iter, bool warm) {
  PolishPlan pl;
  if (sw.no_polish || polish_iters <= 0) return pl;
  const SiteShape& s = rt.site;
  const int nrow = s.M + s.has_peak;
  // the on-chip and the long-horizon polish take over INSIDE the launch, at polish_iters, from a cold start; the wide-site
  // polish runs BEHIND the last pass, cold or warm-started alike
  const bool hand_over = polish_iters < max_iter && !warm;
  const bool lng = hand_over && rt.polish_long_shape && sw.long_polish && polish_long_holds(s.N, rt.t_max, rt.k_sessions, s.Mg, nrow);
  const bool wide = rt.polish_wide_shape && sw.wide_polish && polish_wide_holds(s.N, rt.t_max, rt.k_sessions, s.Mg, nrow);
  if (hand_over && rt.polish_shape) {
    // LDS of a polish workgroup: where the solver kernel runs two workgroups per CU (the headline shape: one column tile,
    // one row tile, one session slot: 77 KB each) the polish takes no more than one of those slots, so that it starts as
    // soon as ANY solver workgroup of a neighbouring stream's launch ends; elsewhere the whole CU
    const bool two_per_cu = rt.tiled && rt.t_max <= 16 && s.MR == 16 && rt.k_sessions == 1;
    const int sess = polish_max_sess(s.N, rt.k_sessions);
    const int blk = polish_blocks_that_fit(s.N, rt.t_max, s.Mg, nrow, sess, two_per_cu ? 76 * 1024 : 160 * 1024);
    if (blk < 2 * nrow * (2 * nrow + 1) / 2) return pl;   // not even one full block
    pl.kind = PolishKind::on_chip;
    pl.max_rows = polish_max_rows(nrow, rt.t_max); pl.max_sess = sess; pl.blk_doubles = blk;
    pl.rows_for_solver = pl.max_rows;
  } else if (lng || wide) {
    // tables for the worst case of the shape, in the workgroup's slab (PolishLongLayout, PolishWideLayout)
    pl.kind = lng ? PolishKind::long_horizon : PolishKind::wide;
    pl.max_rows = polish_long_rows(s.Mg, rt.t_max); pl.max_sess = polish_long_sess(s.N, rt.k_sessions);
    pl.blk_doubles = lng ? polish_long_block_doubles(rt.t_max, s.Mg) : polish_wide_block_doubles(rt.t_max, s.Mg);
    pl.rows_for_solver = pl.max_rows + 8;
  }
  return pl;
}

// workgroups of the polish launch: the slab kernels' own caps; on chip one per CU for a lone launch and a few for a launch of
// the handle's own pipeline streams (a chunk hands a handful of problems over: the launch must not queue for 256 slots behind
// the neighbouring streams' solver launches)
inline int polish_grid(PolishKind kind, int batch, bool own_stream, int cus) {
  if (kind == PolishKind::long_horizon) return polish_long_grid(batch);
  if (kind == PolishKind::wide) return polish_wide_grid(batch);
  return std::max(1, std::min(batch, own_stream ? 32 : cus));
}
// bytes of the slabs of `grid` workgroups (0: the kind keeps its state in LDS)
inline size_t polish_slab_bytes(PolishKind kind, const SiteShape& s, int t_max, int k_sessions, int grid) {
  const int nrow = s.M + s.has_peak;
  if (kind == PolishKind::long_horizon) return (size_t)polish_long_slab_bytes(s.N, t_max, k_sessions, s.Mg, nrow, grid);
  if (kind == PolishKind::wide) return (size_t)polish_wide_slab_bytes(s.N, t_max, k_sessions, s.Mg, nrow, grid);
  return 0;
}

// the counters at the head of a launch's scratch, as indices into int32_t ctr[64]
constexpr int kPolCtrPolishQueue = 0;   // work queue of the polish kernel
constexpr int kPolCtrResumeQueue = 1;   // work queue of the resume launch (on-chip and long-horizon kinds)
constexpr int kPolCtrListLength = 2;    // problems on the list
constexpr int kPolCtrRetired = 3;       // problems the solver launch has finished, for the polish alongside it

// The scratch of one polished launch, as byte offsets: the counters (one 256-byte line); the list int32_t[batch]; the saved
// status int32_t[batch] (wide only); the site-row multipliers double[batch][Mg][Tm] unless the caller wants them anyway;
// the slabs, one per workgroup (long-horizon and wide).  Every region starts on a multiple of 256 bytes; an absent one is
// empty.  `total` is the end of the last.
struct PolishScratch {
  static constexpr size_t kCtrBytes = 256;
  size_t ctr = 0, list = 0, saved = 0, y = 0, slab = 0, total = 0;
  size_t list_bytes = 0;   // of the list's region (and of the saved status')
  PolishScratch(PolishKind kind, int batch, int Mg, int Tm, bool caller_has_y, size_t slab_bytes) {
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const bool slabs = kind == PolishKind::long_horizon || kind == PolishKind::wide;
    list_bytes = up((size_t)batch * sizeof(int32_t));
    list = ctr + kCtrBytes;
    saved = list + list_bytes;
    y = saved + (kind == PolishKind::wide ? list_bytes : 0);
    slab = y + (caller_has_y ? 0 : up((size_t)batch * Mg * Tm * sizeof(double)));
    total = slab + (slabs ? slab_bytes : 0);
  }
};

}  // namespace acnqp
