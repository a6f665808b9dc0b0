// Host side of the C ABI declared in include/acn_qp.h: the extern "C" entry points.  What they decide from a shape is
// in acn_qp_route.hpp, the site upload in acn_qp_site.hpp, the host-buffer entries' chunk pipeline in acn_qp_pipeline.hpp,
// the post-solve entries (duals, pilots, advance, prepare, plant, estimate) and their one staging loop in acn_qp_post.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "acn_qp.h"
#include "acn_qp_launch.hpp"
#include "acn_qp_polplan.hpp"
#include "acn_qp_duals.hpp"
#include "acn_qp_pilots.hpp"
#include "acn_qp_advance.hpp"
#include "acn_qp_advance_vjp.hpp"
#include "acn_qp_prepare.hpp"
#include "acn_qp_plant.hpp"
#include "acn_qp_estimate.hpp"
#include "acn_qp_hold.hpp"
#include "acn_qp_vjp.hpp"
#include "acn_qp_site.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int rc, const std::string& msg) {
  g_last_error = msg;
  return rc;
}

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess)                                                                \
      return fail(ACNQP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
  } while (0)

// grow-only buffer over one pair of allocate / free calls; reserve() frees before it allocates anew (nothing is kept)
template <hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = Alloc(&p, bytes ? bytes : 16);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)Free(p);
    p = nullptr;
    cap = 0;
  }
};
inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
using DevBuf = GrowBuf<device_alloc, hipFree>;
using HostBuf = GrowBuf<pinned_alloc, hipHostFree>;   // pinned host staging

// Grow the device buffers that earlier operations on stream `st` may still use: a buffer that must grow is freed first, so
// the stream is drained before (once, and only if one of them grows).
struct Want { DevBuf* buf; size_t bytes; };
inline hipError_t reserve_behind(hipStream_t st, std::initializer_list<Want> wants) {
  const bool grow = std::any_of(wants.begin(), wants.end(), [](const Want& w) { return w.bytes > w.buf->cap; });
  hipError_t e = grow ? hipStreamSynchronize(st) : hipSuccess;
  for (const Want& w : wants)
    if (e == hipSuccess) e = w.buf->reserve(w.bytes);
  return e;
}

}  // namespace

struct acnqp_handle {
  int device = 0;
  acnqp::SiteShape shape;
  std::vector<double> G, limits;   // host copy in ABI order
  acnqp::SiteDev site;
  static constexpr int kEvRing = 64;               // event pairs of the most recent launches
  hipEvent_t ev_start[kEvRing] = {}, ev_stop[kEvRing] = {};
  long long launches = 0, reported = 0;           // launches recorded / already handed out by acnqp_kernel_times
  long long ordered_launches = 0;                 // launches whose queue order was sorted by launch_order_keys' key (acnqp_ordered_launch_count)
  long long direct_in_last = 0;                   // ... whose lb / ub / q the kernel loaded from the caller's arrays (acnqp_debug_direct_in)
  long long direct_x_last = 0;                    // problems of the last host-entry call whose x the kernel stored into the caller's array (acnqp_debug_direct_x)
  // host-buffer entry points: kSlots pipeline slots, each with its own stream and device staging, so that the
  // H2D copies, the kernel and the D2H copies of successive chunks of a call overlap
  static constexpr int kSlots = 4;
  struct Slot { hipStream_t st = nullptr; DevBuf in, out, tin; } slot[kSlots];   // tin: session-table staging (acnqp_solve_table)
  // pinned mirrors of a call's SMALL per-problem arrays (scalars, session slots; status ... obj): one H2D and one D2H per
  // chunk instead of nine and five per batch of the call -- a stream operation costs tens of microseconds whatever its size,
  // and a step of 64 batches was 960 of them (run_pipeline)
  HostBuf small_in, small_out;
  hipEvent_t h2d_done[kSlots] = {nullptr, nullptr, nullptr, nullptr};   // chunk c's inputs have landed (run_pipeline: the next chunk's copies queue behind them)
  // per launch stream: the kernel workspace (long-horizon, large-site, general-shape kernels) and the launch's small
  // scheduling buffer (queue counter, then sort keys and queue order).  Launches on different streams never share (or
  // regrow) each other's state, and a stream's own launches are ordered by the stream.
  struct Work {
    hipStream_t st; DevBuf buf; DevBuf ord; DevBuf pol; long long used; hipEvent_t last; DevBuf dua;   // pol: the polish's list and multiplier buffer; dua: g of a dual report without z
    hipEvent_t fork = nullptr, join = nullptr;   // the polish alongside a solver launch: where it may start, where it has ended (created on first use)
    DevBuf vjp;                                  // the slabs of a long-horizon backward (acn_qp_vjp_long.hpp)
    void release() {
      if (last) (void)hipEventDestroy(last);
      if (fork) (void)hipEventDestroy(fork);
      if (join) (void)hipEventDestroy(join);
      last = fork = join = nullptr;
      for (DevBuf* b : {&buf, &ord, &pol, &dua, &vjp}) b->release();
    }
  };
  std::vector<Work> work;
  long long work_clock = 0;
  // streams of the CALLER (acnqp_solve_batch_device) beyond the handle's own kSlots: a caller that round-robins one
  // handle over more streams than this pays an event wait + free / malloc per call; 0 < env
  // ACNQP_CALLER_STREAMS <= 256 overrides
  static size_t max_caller_workspaces() {
    static const size_t v = [] {
      const char* e = std::getenv("ACNQP_CALLER_STREAMS");
      const long n = e ? std::atol(e) : 0;
      return (size_t)(n > 0 && n <= 256 ? n : 16);
    }();
    return v;
  }
  Work* work_for(hipStream_t st) {
    for (auto& w : work) if (w.st == st) { w.used = ++work_clock; return &w; }
    // a caller that keeps creating streams must not grow the handle without bound: evict the least recently used
    // entry of a caller stream -- after ITS last launch has finished (the event recorded behind it: that stream may be
    // gone by now), not after the whole device has drained
    bool own = false;
    for (auto& sl : slot) own = own || sl.st == st;
    if (!own) {
      size_t callers = 0, lru = work.size();
      for (size_t k = 0; k < work.size(); ++k) {
        bool mine = false;
        for (auto& sl : slot) mine = mine || sl.st == work[k].st;
        if (mine) continue;
        ++callers;
        if (lru == work.size() || work[k].used < work[lru].used) lru = k;
      }
      if (callers >= max_caller_workspaces()) {
        if (work[lru].last) (void)hipEventSynchronize(work[lru].last);   // (behind the launch's join with the auxiliary stream)
        work[lru].release();
        work.erase(work.begin() + (long)lru);
      }
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    work.push_back(Work{st, DevBuf(), DevBuf(), DevBuf(), ++work_clock, ev, DevBuf()});
    return &work.back();
  }
  int cus = 0;   // compute units of the device (the work-queue launches size their grid from it)
  int32_t* pol_stats = nullptr;   // device counters of the polish kernel, summed over the handle's life (acnqp_polish_stats);
                                  // [16]: problems taken by the launches alongside the solver (acnqp_debug_polish_alongside)
  hipStream_t aux = nullptr;      // the polish launches that run alongside a solver launch (launch_with_polish)
  bool long_polish = false;       // acnqp_set_long_polish: polish_long_shape routes run the long-horizon polish
  bool wide_polish = false;       // acnqp_set_wide_polish: polish_wide_shape routes run the wide-site polish behind the solver launch
  bool long_vjp = false;          // acnqp_set_long_vjp: the vjp entries serve horizons 33 ... 288 too (acn_qp_vjp_long.hpp)
  // the post-solve host entries' device staging (acn_qp_post.hpp: the whole-call arrays and one chunk).  ONE buffer for
  // the three: each runs on slot[0].st, synchronises it before reserve() and returns synchronised
  DevBuf post_stage;
};

namespace {

static_assert(acnqp::kRouteMaxK == acnqp::kMaxK, "acn_qp_route.hpp restates the on-chip kernels' session slots");

// The diagnostic switches of the routing table (acn_qp_route.hpp) from the environment: the wave switches once per
// process, ACNQP_NO_LONG and ACNQP_LDS_LONG at every call.
acnqp::RouteSwitches route_switches() {
  static const bool no_wave = std::getenv("ACNQP_NO_WAVE") != nullptr;
  static const bool no_wave2 = std::getenv("ACNQP_NO_WAVE2") != nullptr;
  static const int min_batch = std::getenv("ACNQP_WAVE_MIN_BATCH") ? std::atoi(std::getenv("ACNQP_WAVE_MIN_BATCH")) : 1;
  acnqp::RouteSwitches sw;
  sw.no_wave = no_wave; sw.no_wave2 = no_wave2; sw.wave_min_batch = min_batch;
  sw.no_long = std::getenv("ACNQP_NO_LONG") != nullptr;
  const char* e = std::getenv("ACNQP_LDS_LONG");
  sw.lds_long = !(e && std::atoi(e) == 0);
  return sw;
}
acnqp::Route route_of(const acnqp_handle* h, int t_max, int k_sessions, int batch) {
  return acnqp::route_for(h->shape, t_max, k_sessions, batch, route_switches());
}

// the kernels' own size formulas, for the routing table (which includes no kernel text)
struct Kernels {
  static int wave_accel() { return acnqp::wave_accel_columns(); }
  static int tiled_accel(int MT, int CT, int NP, int K) { int single = 0; return acnqp::accel_capacity_best(4, MT, CT, NP, K, &single); }
  static int stream_accel() { return acnqp::kStreamAccelMax; }   // ring in its workspace
  static int long_accel() { return acnqp::kLongAccelMax; }       // ring in its workspace
  static int general_accel() { return acnqp::kGenAccelMax; }     // ring in its workspace
  static long long stream_workspace(int NP, int CT, int K, int MT, int accel) { return acnqp::stream_workspace(NP, CT, K, MT, accel); }
  static long long long_workspace(int NP, int t_max, int K, int MT, int accel) { return acnqp::long_workspace(NP, acnqp::long_tiles(t_max), K, MT, accel); }
};

// The polish of a launch (acn_qp_polplan.hpp: whether, by which kernel, with which tables) under the options' polish_iters and
// max_iter, cold or warm-started.  ACNQP_NO_POLISH (diagnostic, read once per process): none.  (The polish phase runs behind
// the solver launch; on throughput-bound launches it adds its rounds to the launch's end, DESIGN.md 2.3 has the price.)
acnqp::PolishPlan polish_plan_of(const acnqp_handle* h, const acnqp::Route& rt, int polish_iters, int max_iter, bool warm) {
  static const bool no_polish = std::getenv("ACNQP_NO_POLISH") != nullptr;
  acnqp::PolishSwitches sw;
  sw.no_polish = no_polish; sw.long_polish = h->long_polish; sw.wide_polish = h->wide_polish;
  return acnqp::polish_plan(rt, sw, polish_iters, max_iter, warm);
}

// acnqp_solve_batch_device with the pipeline's knowledge of what comes after the launch (nothing_follows: launch_with_polish)
// and of the direct paths (ht: device arrays of host addresses -- x: TiledArgs::x_host, where the schedules go besides r->x;
// lb, ub, q: TiledArgs::lb_host ..., where the kernel finds the inputs that p->lb / ub / q do not hold yet)
struct HostTables {
  double* const* x = nullptr;
  const double* const* lb = nullptr;   // (all three, or none)
  const double* const* ub = nullptr;
  const double* const* q = nullptr;
};
int solve_batch_device(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, acnqp_results* r, hipStream_t st, bool nothing_follows,
                       const HostTables& ht = HostTables());

}  // namespace

#include "acn_qp_pipeline.hpp"
#include "acn_qp_post.hpp"
extern "C" {

int32_t acnqp_abi_version(void) { return ACNQP_ABI_VERSION; }

int32_t acnqp_route(acnqp_handle* h, int32_t t_max, int32_t k_sessions, int32_t batch, int32_t* polish) {
  if (polish) *polish = 0;
  if (!h || t_max < 1 || t_max > 4096 || k_sessions < 1 || k_sessions > 4096 || batch < 1) return 0;
  const acnqp::Route r = route_of(h, t_max, k_sessions, batch);
  acnqp_options o;   // (the polish flag: what a launch with the DEFAULT options does)
  acnqp_default_options(&o);
  if (polish) *polish = polish_plan_of(h, r, o.polish_iters, o.max_iter, false).kind != acnqp::PolishKind::none ? 1 : 0;
  return r.family;
}

const char* acnqp_last_error(void) { return g_last_error.c_str(); }

void acnqp_default_options(acnqp_options* o) {
  if (!o) return;
  o->eps_abs = 1e-8;
  o->eps_rel = 1e-8;
  o->max_iter = 20000;
  o->check_every = 20;
  o->adapt_every = 20;
  o->rho = 0.02;
  o->sigma = 1e-6;
  o->alpha = 1.4;
  o->adapt_tol = 3.0;
  o->reg_rel = 0.06;
  o->precision = 64;
  o->accel_mem = 5;
  o->stall_iters = 3000;
  o->retry_passes = 2;
  o->retry_max_iter = 8000;
  o->polish_iters = 800;
  o->retry_rho = 0.5;
  o->inaccurate_floor = 1e-5;
  o->polish_stall = 0;
}

int acnqp_create(const acnqp_site* site, int32_t device_id, acnqp_handle** out) {
  if (!site || !out) return fail(ACNQP_ERR_INVALID, "acnqp_create: null argument");
  *out = nullptr;
  const int N = site->n_evse, M = site->n_infra, Mg = site->n_rows;
  if (N < 1 || N > 1024)
    return fail(ACNQP_ERR_INVALID, "acnqp_create: n_evse must be in [1, 1024]");
  if (site->cone != ACNQP_CONE_LINEAR && site->cone != ACNQP_CONE_SOC)
    return fail(ACNQP_ERR_INVALID, "acnqp_create: cone must be ACNQP_CONE_LINEAR or ACNQP_CONE_SOC");
  const int expect = (site->cone == ACNQP_CONE_SOC ? 2 * M : M) + (site->has_peak ? 1 : 0) + (site->has_flat ? 1 : 0) + (site->has_max ? 1 : 0);
  if (M < 0 || Mg != expect || Mg > 48)
    return fail(ACNQP_ERR_INVALID, "acnqp_create: n_rows inconsistent with n_infra/cone/has_peak/has_flat/has_max or > 48");
  // the kernels' row tiles: SOC pads its 2M rows to 8*ceil(M/4), and the padded count must fit 48
  const int padded = acnqp::padded_rows(site->cone, M, site->has_peak, site->has_flat, site->has_max);
  if (padded > 48)
    return fail(ACNQP_ERR_INVALID, "acnqp_create: " + std::to_string(padded) + " site rows after padding (SOC: 8*ceil(n_infra/4) "
                                   "+ peak/flat/max rows) > 48, the padded limit");
  if (Mg > 0 && !site->G) return fail(ACNQP_ERR_INVALID, "acnqp_create: G is null");
  if (M > 0 && !site->limits) return fail(ACNQP_ERR_INVALID, "acnqp_create: limits is null");
  for (int j = 0; j < M; ++j)
    if (!(site->limits[j] >= 0)) return fail(ACNQP_ERR_INVALID, "acnqp_create: limits must be >= 0");

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(ACNQP_ERR_NO_DEVICE, "acnqp_create: no HIP device visible");
  if (device_id < 0 || device_id >= ndev) return fail(ACNQP_ERR_INVALID, "acnqp_create: bad device_id");
  HIP_TRY(hipSetDevice(device_id));

  acnqp_handle* h = new acnqp_handle();
  h->device = device_id;
  h->shape = acnqp::site_shape(N, M, site->cone, site->has_peak, site->has_flat, site->has_max);
  if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || h->cus < 1) h->cus = 256;
  h->G.assign(site->G, site->G + (size_t)Mg * N);
  h->limits.assign(site->limits, site->limits + M);
  hipError_t e = hipSuccess;
  for (int k = 0; k < acnqp_handle::kEvRing && e == hipSuccess; ++k) {
    e = hipEventCreate(&h->ev_start[k]);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_stop[k]);
  }
  for (int k = 0; k < acnqp_handle::kSlots && e == hipSuccess; ++k) {
    e = hipStreamCreateWithFlags(&h->slot[k].st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->h2d_done[k], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    std::string msg = std::string("acnqp_create: ") + hipGetErrorString(e);
    acnqp_destroy(h);
    return fail(ACNQP_ERR_HIP, msg);
  }
  std::string err;
  const int rc = acnqp::build_site_dev(&h->shape, h->G, h->limits, &h->site, &err);
  if (rc != ACNQP_OK) { acnqp_destroy(h); return fail(rc, err); }
  if (hipMalloc((void**)&h->pol_stats, 32 * sizeof(int32_t)) != hipSuccess || hipMemset(h->pol_stats, 0, 32 * sizeof(int32_t)) != hipSuccess ||
      hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) != hipSuccess) {
    acnqp_destroy(h);
    return fail(ACNQP_ERR_HIP, "acnqp_create: polish counters and stream");
  }
  *out = h;
  return ACNQP_OK;
}

void acnqp_destroy(acnqp_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  h->site.release();
  for (int k = 0; k < acnqp_handle::kEvRing; ++k) {
    if (h->ev_start[k]) (void)hipEventDestroy(h->ev_start[k]);
    if (h->ev_stop[k]) (void)hipEventDestroy(h->ev_stop[k]);
  }
  for (auto& sl : h->slot) {
    if (sl.st) { (void)hipStreamSynchronize(sl.st); (void)hipStreamDestroy(sl.st); }
    for (DevBuf* b : {&sl.in, &sl.out, &sl.tin}) b->release();
  }
  if (h->aux) { (void)hipStreamSynchronize(h->aux); (void)hipStreamDestroy(h->aux); }
  h->small_in.release();
  h->small_out.release();
  for (auto& ev : h->h2d_done) if (ev) (void)hipEventDestroy(ev);
  for (auto& w : h->work) w.release();
  h->post_stage.release();
  if (h->pol_stats) (void)hipFree(h->pol_stats);
  delete h;
}

// NaN by its bits: this file is compiled with -fno-honor-nans, under which `!(v >= 0)` is folded to `v < 0` and lets a
// NaN option through the comparisons below.
static bool is_nan(double v) {
  uint64_t u;
  std::memcpy(&u, &v, sizeof u);
  return (u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

static int check_problem_shapes(const acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o,
                                const acnqp_results* r) {
  if (!h || !p || !o || !r) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: null argument");
  if (p->batch < 0) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: negative batch");
  if (p->batch == 0) return ACNQP_OK;
  if (p->t_max < 1 || p->t_max > 4096)
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: t_max must be in [1, 4096]");
  if (p->k_sessions < 1 || p->k_sessions > 4096)
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: k_sessions must be in [1, 4096]");
  if (!p->horizon || !p->lb || !p->ub || !p->q || !p->pdiag || !p->s_off || !p->s_len || !p->s_cap || !p->s_eq)
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: null problem array");
  if (h->shape.has_peak && !p->peak) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: site has a peak row but peak is null");
  if (h->shape.has_flat && !p->lf) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: site has a flat row but lf is null");
  if (h->shape.has_max && (!p->dc || !p->dfloor)) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: site has a max row but dc/dfloor is null");
  if ((p->warm_x == nullptr) != (p->warm_y == nullptr))
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: warm_x and warm_y must be given together");
  if (!r->x || !r->status || !r->iters || !r->pri_res || !r->dua_res || !r->obj)
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: null result array");
  for (double v : {o->eps_abs, o->eps_rel, o->rho, o->sigma, o->alpha, o->adapt_tol, o->reg_rel, o->retry_rho, o->inaccurate_floor})
    if (is_nan(v)) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: invalid option value");
  if (!(o->eps_abs >= 0) || !(o->eps_rel >= 0) || o->max_iter < 1 || o->check_every < 1 || !(o->rho > 0) ||
      !(o->sigma >= 0) || !(o->alpha > 0 && o->alpha < 2) || !(o->adapt_tol > 1) || !(o->reg_rel >= 0) ||
      o->adapt_every < 0 || o->polish_iters < 0 || o->polish_stall < 0 || o->stall_iters < 0 || o->retry_passes < 0 || o->retry_passes > 8 || o->retry_max_iter < 1 ||
      !(o->retry_rho > 0) || !(o->inaccurate_floor >= 0))
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: invalid option value");
  if (o->precision != 64)
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_batch: precision must be 64 (the fp32 loop was removed: it missed the "
                                   "1e-4 rate tolerance on weakly convex problems and was not faster; DESIGN.md section 3)");
  return ACNQP_OK;
}

// ---- acnqp_solve_batch_device, step by step ------------------------------------------------------------------------------
namespace {

// the kernel arguments a launch takes from the handle, the problems, the results and the options (schedule, workspace
// and polish fields: the steps below)
acnqp::TiledArgs tiled_args(const acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, const acnqp_results* r, hipStream_t st) {
  const acnqp::SiteShape& s = h->shape;
  const acnqp::SiteDev* d = &h->site;
  acnqp::TiledArgs a;
  a.B = p->batch; a.N = s.N; a.Tm = p->t_max; a.K = p->k_sessions; a.NP = s.NP(); a.MR = s.MR;
  a.G = d->G; a.Ghat = d->Ghat; a.Q = d->Q; a.lam = d->lam; a.rowlim = d->rowlim; a.rowtype = d->rowtype;
  a.fragG = d->fragG; a.fragQ = d->fragQ; a.fragG2 = d->fragG2; a.fragQ2 = d->fragQ2;
  a.horizon = p->horizon; a.lb = p->lb; a.ub = p->ub; a.q = p->q; a.pdiag = p->pdiag;
  a.s_off = p->s_off; a.s_len = p->s_len; a.s_cap = p->s_cap; a.s_eq = p->s_eq; a.peak = s.has_peak ? p->peak : nullptr;
  a.lf = s.has_flat ? p->lf : nullptr;
  a.dc = s.has_max ? p->dc : nullptr;
  a.dfloor = s.has_max ? p->dfloor : nullptr;
  a.warm_x = (p->warm_x && p->warm_y) ? p->warm_x : nullptr;
  a.warm_y = (p->warm_x && p->warm_y) ? p->warm_y : nullptr;
  a.y_out = r->y;
  a.rowabi = d->rowabi; a.rowscale = d->rowscale; a.Mg = s.Mg;
  a.x = r->x; a.status = r->status; a.iters = r->iters; a.pri = r->pri_res; a.dua = r->dua_res; a.obj = r->obj;
  a.eps_abs = o->eps_abs; a.eps_rel = o->eps_rel; a.rho0 = o->rho; a.sigma = o->sigma; a.alpha = o->alpha;
  a.adapt_tol = o->adapt_tol; a.reg_rel = o->reg_rel;
  a.max_iter = o->max_iter; a.check_every = o->check_every; a.adapt_every = o->adapt_every;
  a.peak_scale = d->peak_scale; a.flat_scale = d->flat_scale; a.max_scale = d->max_scale;
  a.accel_mem = std::max(0, o->accel_mem);
  a.stall_iters = o->stall_iters; a.retry_passes = o->retry_passes; a.retry_max_iter = o->retry_max_iter;
  a.retry_rho = o->retry_rho; a.inacc_floor = o->inaccurate_floor;
  a.pbuf_single = 0;
  a.order = nullptr;
  a.queue = nullptr;
  // launches of the handle's own pipeline streams (the host-buffer entries: several launches in flight) keep their
  // workgroups only for a few problems each; a launch on a caller's stream is fully persistent
  bool own = false;
  for (auto& sl : h->slot) own = own || sl.st == st;
  a.grid_oversub = own ? 4 : 1;
  a.polish_iters = 0; a.polish_stall = 0; a.resume = 0; a.y_for_polish_only = 0; a.pol_rows = 0; a.pol_list = nullptr; a.pol_count = nullptr; a.pol_retired = nullptr; a.count_dev = nullptr;
  a.x_host = nullptr;
  a.lb_host = nullptr; a.ub_host = nullptr; a.q_host = nullptr;
  return a;
}

// The work queue and the launch order, in this stream's scheduling buffer, and the grid cap that follows from them.
// The work queue serves the kernels whose state is ON CHIP (register-resident, LDS-resident long-horizon): their
// launches end on their slowest workgroup slot, and levelling the slots is worth 7-10 % (headline lone launch 28.8 ->
// 26.9 ms, jpl52 x 24 x 4,096 67.2 -> 60.6 ms).  The kernels that stream their state through HBM are bandwidth-bound
// across the whole chip: a slot that ends early leaves its bandwidth to the others, and the static schedule measured
// the same or better (configs[4] leg 432 vs 434-438 ms, 54 x 144 x 2,048 237-243 vs 247-248 ms; gpurun_out/r4c):
// they keep one workgroup per problem.
// The launch-order keys of the device-resident problems p (which route rt serves) into keys[p->batch], on st: the
// congestion key of order_keys_kernel, or the session count.  The session count is the key
//  * of a shape beyond that kernel's LDS budget (order_key_waves),
//  * of the four-wave route (two row tiles x horizon 13-24), the one ordered leg that measured a LOSS under the
//    congestion key (jpl52 x 24 x 4,096, five runs each: 43.52-43.69 ms by sessions, 43.77-43.99 ms by congestion;
//    profiles/order_key_ab.json),
//  * under ACNQP_ORDER_KEY=sessions (diagnostic, read once per process; `overload` names the default),
//  * of a launch whose lb / ub / q are not on the device when the key kernel would run (small_only: the direct path for
//    the inputs, acn_qp_pipeline.hpp): the congestion key reads ub.
// By shape, route and where the inputs are, never by batch.
hipError_t launch_order_keys(acnqp_handle* h, const acnqp::Route& rt, const acnqp_problems* p, hipStream_t st, int32_t* keys, bool small_only = false) {
  static const bool by_sessions = [] { const char* e = std::getenv("ACNQP_ORDER_KEY"); return e && std::strcmp(e, "sessions") == 0; }();
  const acnqp::SiteShape& s = h->shape;
  const int g_rows = s.cone == ACNQP_CONE_SOC ? 2 * s.M : s.M;
  const int waves = by_sessions || small_only || rt.family == ACNQP_ROUTE_WAVE4 ? 0 : order_key_waves((size_t)s.N, (size_t)p->t_max, (size_t)g_rows);
  if (waves == 0) {
    hipLaunchKernelGGL(session_keys_kernel, dim3((p->batch + 3) / 4), dim3(256), 0, st, p->s_len, p->k_sessions * s.N, p->batch, keys);
    return hipGetLastError();
  }
  OrderKeyArgs ka;
  ka.B = p->batch; ka.N = s.N; ka.Tm = p->t_max; ka.K = p->k_sessions; ka.M = s.M; ka.soc = s.cone == ACNQP_CONE_SOC; ka.has_peak = s.has_peak;
  ka.lb = p->lb; ka.ub = p->ub; ka.s_cap = p->s_cap; ka.peak = p->peak; ka.G = h->site.Gabi; ka.limits = h->site.limabi;
  ka.s_off = p->s_off; ka.s_len = p->s_len; ka.horizon = p->horizon; ka.keys = keys;
  const size_t lds = ((size_t)g_rows * s.N + (size_t)waves * s.N * p->t_max) * sizeof(double);
  const hipError_t e = acnqp::ensure_dynamic_lds(reinterpret_cast<const void*>(order_keys_kernel), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(order_keys_kernel, dim3((p->batch + waves - 1) / waves), dim3(64 * waves), lds, st, ka);
  return hipGetLastError();
}

int schedule_launch(acnqp_handle* h, acnqp_handle::Work* wk, const acnqp::Route& rt, const acnqp_problems* p, hipStream_t st, acnqp::TiledArgs* a) {
  static const bool no_order = std::getenv("ACNQP_NO_ORDER") != nullptr;   // diagnostic: queue position b = problem b
  static const bool no_queue_env = std::getenv("ACNQP_NO_QUEUE") != nullptr;   // diagnostic: the static schedule (workgroup w = position w)
  static const bool queue_all = std::getenv("ACNQP_QUEUE_ALL") != nullptr;     // diagnostic: the queue for the streaming kernels too
  const bool no_queue = no_queue_env || !(rt.on_chip || queue_all);
  // (an order only for separable objectives: with a load-flattening or demand-charge row the coupling, which neither the
  //  session count nor the overloaded cells of the greedy schedule see, sets the iteration count -- by sessions the
  //  configs[4] leg was 10 % SLOWER than in the natural order)
  const bool want_order = p->batch >= kOrderMinBatch && !no_order && !h->shape.has_flat && !h->shape.has_max;
  if (!no_queue || want_order) {
    // scheduling buffer of this stream: [0] the queue counter (its own 256-byte line), then keys[B], order[B]
    const size_t need = 256 + (want_order ? (size_t)p->batch * 2 * sizeof(int32_t) : 0);
    HIP_TRY(reserve_behind(st, {{&wk->ord, need}}));
    if (!no_queue) {
      a->queue = static_cast<int32_t*>(wk->ord.p);
      HIP_TRY(hipMemsetAsync(a->queue, 0, sizeof(int32_t), st));
    }
    if (want_order) {
      int32_t* keys = static_cast<int32_t*>(wk->ord.p) + 64;
      int32_t* order = keys + p->batch;
      HIP_TRY(launch_order_keys(h, rt, p, st, keys, a->lb_host != nullptr));
      hipLaunchKernelGGL(order_sort_kernel, dim3(1), dim3(kOrderKeys), 0, st, keys, p->batch, order);
      a->order = order;
      h->ordered_launches++;
    }
  }
  // workgroups of a work-queue launch that get a workspace of their own (the kernels that stream their state): at most
  // two resident workgroups per CU (no streaming kernel has more); the launchers cap their grid at it
  static const bool ws_per_problem = std::getenv("ACNQP_WS_PER_PROBLEM") != nullptr;   // diagnostic
  a->ws_by_slot = a->queue && !ws_per_problem ? 1 : 0;
  a->grid_cap = a->ws_by_slot ? std::min(p->batch, 2 * h->cus) : p->batch;
  return ACNQP_OK;
}

// The workspace of the families that stream their state (large-site, long-horizon, general-shape: Route::workspace_doubles
// per workgroup of the grid; not graph-capturable: it may allocate).  The two MFMA kernels take no more Anderson columns
// than their ring holds.
struct Workspace { void* p = nullptr; long long per_problem = 0; };
int reserve_workspace(acnqp_handle::Work* wk, const acnqp::Route& rt, hipStream_t st, acnqp::TiledArgs* a, Workspace* ws) {
  if (rt.tiled) return ACNQP_OK;
  if (rt.stream || rt.lng) a->accel_mem = std::min(a->accel_mem, rt.accel_cap<Kernels>());
  ws->per_problem = rt.workspace_doubles<Kernels>(a->accel_mem);
  const size_t need = (size_t)ws->per_problem * a->grid_cap * sizeof(double);
  HIP_TRY(reserve_behind(st, {{&wk->buf, need}}));
  ws->p = wk->buf.p;
  return ACNQP_OK;
}

// The eigen extent of the wave kernel's instantiation for this handle's site (acn_qp_rank.hpp; 0: the full one).
// ACNQP_WAVE_FULL_RANK=1 (diagnostic, read once per process): the full extent for every site -- the kernel as it was.
int wave_extent_of(const acnqp_handle* h) {
  static const bool full_rank = std::getenv("ACNQP_WAVE_FULL_RANK") != nullptr;
  return acnqp::wave_eig_extent(h->site.eig_ksteps, full_rank);
}

// The EVSE k-steps of P = Ghat r0 in the wave kernel's instantiation for this handle's site (acn_qp_rank.hpp).
// ACNQP_WAVE_FULL_EVSE=1 (diagnostic, read once per process): all 16 for every site -- the kernel as it was.
int wave_evse_extent_of(const acnqp_handle* h) {
  static const bool full_evse = std::getenv("ACNQP_WAVE_FULL_EVSE") != nullptr;
  return acnqp::wave_evse_extent(h->shape.N, full_evse);
}

hipError_t launch_solver(const acnqp_handle* h, const acnqp::Route& rt, const acnqp::TiledArgs& aa, const Workspace& ws, hipStream_t st) {
  if (rt.wv > 0) {
    acnqp::WaveSite w;
    w.Ghat = h->site.GhatW; w.lam = h->site.lamW; w.fragQ = h->site.fragQW; w.extent = wave_extent_of(h);
    w.evse_ksteps = wave_evse_extent_of(h);
    return acnqp::launch_wave(aa, w, st);
  }
  if (rt.tiled) return rt.t_max <= 16 ? acnqp::launch_tiled_ct1(aa, st) : acnqp::launch_tiled_ct2(aa, st);
  if (rt.stream || rt.lng) {
    acnqp::StreamArgs sa;
    sa.t = aa; sa.work = static_cast<double*>(ws.p); sa.ws_per_problem = ws.per_problem;
    return rt.stream ? acnqp::launch_stream(sa, st) : acnqp::launch_long(sa, st, rt.lds);
  }
  // workgroup size by problem size: the plain loops are latency-bound, more threads per problem hide more of it
  const long long nvar = (long long)rt.site.N * rt.t_max;
  const int nt = nvar <= 4096 ? 256 : (nvar <= 12288 ? 512 : 1024);
  acnqp::GeneralArgs ga;
  ga.t = aa; ga.work = ws.p; ga.ws_per_problem = ws.per_problem; ga.pair_stride = 4;
  return acnqp::launch_general(ga, nt, st);
}

// The direct path for x (acn_qp_pipeline.hpp), the handed-over problems: a problem on the polish's list gets its final
// schedule from the polish kernel or from the resume launch, so behind the two this kernel copies x of every listed
// problem to its host destination (null: none), in flat order like the solver's own stores.  list[0 .. *count) holds the
// problems (every entry published: the solver launch has ended); a handful per chunk.
__global__ __launch_bounds__(256) void pol_x_to_host_kernel(const int32_t* list, const int32_t* count, int B, int nv, const double* x,
                                                            double* const* x_host) {
  const int n = min(*count, B);
  for (int pos = blockIdx.x; pos < n; pos += gridDim.x) {
    const int b = list[pos];
    if (b < 0 || b >= B) continue;
    double* const dst = x_host[b];
    if (dst == nullptr) continue;
    for (int k = threadIdx.x; k < nv; k += blockDim.x) dst[k] = x[(size_t)b * nv + k];
  }
}

// The scratch of a polished launch (PolishScratch, acn_qp_polplan.hpp) in this stream's buffer, reserved behind the stream's
// earlier launches, its counters cleared on `st`: the regions as pointers (saved: the wide kind's; y: the caller's array
// where it gives one; slab: the long-horizon and wide kinds') and the polish launch's grid.
struct PolishBuffers { int32_t *ctr, *list, *saved; double *y, *slab; size_t list_bytes; int grid; };
int reserve_polish(acnqp_handle* h, acnqp_handle::Work* wk, const acnqp::PolishPlan& pl, const acnqp::TiledArgs& a, const acnqp_problems* p,
                   const acnqp_results* r, hipStream_t st, PolishBuffers* pb) {
  const acnqp::SiteShape& s = h->shape;
  pb->grid = acnqp::polish_grid(pl.kind, p->batch, a.grid_oversub > 1, h->cus);
  const acnqp::PolishScratch sc(pl.kind, p->batch, s.Mg, p->t_max, r->y != nullptr,
                                acnqp::polish_slab_bytes(pl.kind, s, p->t_max, p->k_sessions, pb->grid));
  HIP_TRY(reserve_behind(st, {{&wk->pol, sc.total}}));
  char* base = static_cast<char*>(wk->pol.p);
  pb->ctr = reinterpret_cast<int32_t*>(base + sc.ctr);
  pb->list = reinterpret_cast<int32_t*>(base + sc.list);
  pb->saved = reinterpret_cast<int32_t*>(base + sc.saved);
  pb->y = r->y ? r->y : reinterpret_cast<double*>(base + sc.y);
  pb->slab = pl.kind == acnqp::PolishKind::on_chip ? nullptr : reinterpret_cast<double*>(base + sc.slab);
  pb->list_bytes = sc.list_bytes;
  HIP_TRY(hipMemsetAsync(pb->ctr, 0, acnqp::PolishScratch::kCtrBytes, st));
  return ACNQP_OK;
}

// The arguments of the polish kernel of plan `pl` over the list in `pb`, as a serial launch behind the solver (the
// launch alongside sets its own: alongside, retired, max_polls, taken).
// (expected: the problems the FIRST launch serves -- its queue_length is the batch, count_dev being null there; only the
//  resume launch runs over a shorter list.  A first launch over fewer problems would leave the launch alongside polling
//  until its bound)
acnqp::PolishArgs polish_args(const acnqp_handle* h, const acnqp::PolishPlan& pl, const PolishBuffers& pb, const acnqp_problems* p,
                              const acnqp_options* o, const acnqp_results* r) {
  const acnqp::SiteShape& s = h->shape;
  const acnqp::SiteDev* d = &h->site;
  acnqp::PolishArgs pa;
  pa.B = p->batch; pa.N = s.N; pa.Tm = p->t_max; pa.K = p->k_sessions; pa.M = s.M; pa.Mg = s.Mg; pa.cone = s.cone;
  pa.has_peak = s.has_peak; pa.max_rows = pl.max_rows; pa.blk_doubles = pl.blk_doubles; pa.max_sess = pl.max_sess;
  pa.G = d->Gabi; pa.limits = d->limabi;
  pa.horizon = p->horizon; pa.lb = p->lb; pa.ub = p->ub; pa.q = p->q; pa.pdiag = p->pdiag;
  pa.s_off = p->s_off; pa.s_len = p->s_len; pa.s_cap = p->s_cap; pa.s_eq = p->s_eq; pa.peak = s.has_peak ? p->peak : nullptr;
  pa.x = r->x; pa.y = pb.y; pa.status = r->status; pa.iters = r->iters; pa.pri = r->pri_res; pa.dua = r->dua_res; pa.obj = r->obj;
  pa.list = pb.list; pa.count = pb.ctr + acnqp::kPolCtrListLength; pa.queue = pb.ctr + acnqp::kPolCtrPolishQueue;
  pa.stats = h->pol_stats; pa.reg_rel = o->reg_rel;
  pa.alongside = 0; pa.expected = p->batch; pa.retired = nullptr; pa.max_polls = 0; pa.taken = nullptr;
  return pa;
}

// ---- the polish (acn_qp_polish.hpp): small sites, separable objective, served by an on-chip kernel ------------------
// solver kernel (pass 0 up to polish_iters iterations; what has not converged by then is listed) -> polish kernel over
// the list -> solver kernel again over the list for what the polish gave up on (from scratch, with the retry passes:
// the answer it had before there was a polish).  Three launches on the stream, the last two nearly empty as a rule.
// pl: the launch's plan, on_chip or long_horizon (acn_qp_polish_long.hpp: the same sequence with that kernel).
//
// The problems that are handed over are the launch's longest-running ones, and the chip thins out for milliseconds before
// its last straggler ends: where NOTHING FOLLOWS the launch (a caller's stream; the last chunk of a pipelined call) a
// second polish launch runs ALONGSIDE the solver, on the handle's auxiliary stream, and takes the hand-overs as they are
// published (acn_qp_polclaim.hpp) on the CUs the solver's retired workgroups leave.  The serial launches stay as they
// are: they find the list drained, or finish what the launch alongside left.  Wave kernel with a work queue only (its
// hand-over publishes inside the launch and it counts its finished problems: TiledArgs::pol_retired).  Intermediate chunks
// of a pipelined call do without: their serial polish already runs under the next chunk's solver, and spinning workgroups
// would hold CUs that chunk wants.  ACNQP_NO_POLISH_ALONGSIDE=1 (diagnostic, once per process): never.
int launch_with_polish(acnqp_handle* h, acnqp_handle::Work* wk, const acnqp::Route& rt, const acnqp::TiledArgs& a, const Workspace& ws,
                       const acnqp::PolishPlan& pl, const acnqp_problems* p, const acnqp_options* o, const acnqp_results* r, hipStream_t st,
                       bool nothing_follows, hipError_t* e) {
  static const bool no_alongside = std::getenv("ACNQP_NO_POLISH_ALONGSIDE") != nullptr;
  // looks at the list a workgroup alongside makes per claim (an empty one costs about a microsecond: the default outlasts
  // every launch the project times by seconds); 0: every one of them leaves at once, without a look
  static const long long along_polls = [] {
    const char* v = std::getenv("ACNQP_POLISH_ALONGSIDE_SPINS");
    const long long n = v ? std::atoll(v) : (1ll << 21);
    return n < 0 ? 0ll : n;
  }();
  static const int along_grid = [] {   // diagnostic: workgroups of the launch alongside
    const char* v = std::getenv("ACNQP_POLISH_ALONGSIDE_GRID");
    const int n = v ? std::atoi(v) : 0;
    return n > 0 && n <= 256 ? n : 16;
  }();
  // (not the two-row-tile route of horizons <= 12, ACNQP_ROUTE_WAVE3: measured a LOSS there -- configs[3] site 3, 1,024
  //  problems: 7.20-7.36 ms without, 8.02-8.18 ms with; two rounds of problems on 512 slots hand half their stragglers over in
  //  mid-launch, and 16 workgroups then work through a list that the serial launch spreads over the chip)
  // (nor the long-horizon polish, on ACNQP_ROUTE_WAVE5 either: it runs as a serial launch only)
  const bool lng = pl.kind == acnqp::PolishKind::long_horizon;
  const bool alongside = nothing_follows && !no_alongside && rt.wv > 0 && rt.wv != 3 && a.queue != nullptr && !lng;
  PolishBuffers pb;
  const int rc = reserve_polish(h, wk, pl, a, p, r, st, &pb);
  if (rc != ACNQP_OK) return rc;
  int32_t* const list = pb.list;
  int32_t* const count = pb.ctr + acnqp::kPolCtrListLength;
  if (alongside) {
    HIP_TRY(hipMemsetAsync(list, 0xff, pb.list_bytes, st));   // -1: not published
    if (!wk->fork) HIP_TRY(hipEventCreateWithFlags(&wk->fork, hipEventDisableTiming));
    if (!wk->join) HIP_TRY(hipEventCreateWithFlags(&wk->join, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(wk->fork, st));   // counters and list are set: from here on the launch alongside may run
  }
  acnqp::TiledArgs a1 = a;
  a1.polish_iters = o->polish_iters - o->polish_iters % std::max(1, o->check_every);   // the exit is taken at a residual check
  if (a1.polish_iters < o->check_every) a1.polish_iters = o->check_every;
  a1.pol_list = list; a1.pol_count = count; a1.y_out = pb.y; a1.pol_rows = pl.rows_for_solver;
  // (measured, wave kernel: the early hand-over takes 5 % off the headline launch and 23 % off configs[3] site 0, and hands
  //  ten times as many problems to the polish -- one 256-batch per call 81 -> 62 k QP/s, the table path 654 -> 580 k: off
  //  by default; options.polish_stall, ABI v9, is the caller's switch, the environment variable the diagnostic one)
  static const int early = std::getenv("ACNQP_EARLY_HANDOVER") ? std::atoi(std::getenv("ACNQP_EARLY_HANDOVER")) : 0;   // diagnostic: the window (1: polish_iters / 4)
  a1.polish_stall = early > 1 ? early : (early == 1 ? std::max(o->check_every, a1.polish_iters / 4) : o->polish_stall);
  a1.y_for_polish_only = r->y ? 0 : 1;
  a1.pol_retired = alongside ? pb.ctr + acnqp::kPolCtrRetired : nullptr;
  *e = launch_solver(h, rt, a1, ws, st);
  if (*e == hipSuccess) {
    acnqp::PolishArgs pa = polish_args(h, pl, pb, p, o, r);
    pa.retired = pb.ctr + acnqp::kPolCtrRetired; pa.max_polls = along_polls; pa.taken = h->pol_stats + 16;
    if (alongside) {
      // no host synchronisation; nothing the launch alongside waits for is queued behind it: the solver counts its own
      // finished problems, and every poll is bounded
      acnqp::PolishArgs pc = pa;
      pc.alongside = 1;
      // (error paths: a failed launch alongside is reported through *e like any launch, after the join below -- the two
      //  streams are joined whether it ran or not; a HIP_TRY that returns here fails the call with the solver launch
      //  already on `st` and at most the fork wait on `aux`: nothing on either stream waits for something that never comes)
      HIP_TRY(hipStreamWaitEvent(h->aux, wk->fork, 0));
      *e = acnqp::launch_polish(pc, along_grid, h->aux);
      HIP_TRY(hipEventRecord(wk->join, h->aux));
      HIP_TRY(hipStreamWaitEvent(st, wk->join, 0));
    }
    if (*e == hipSuccess) *e = lng ? acnqp::launch_polish_long(pa, pb.slab, pb.grid, st) : acnqp::launch_polish(pa, pb.grid, st);
  }
  if (*e == hipSuccess) {
    acnqp::TiledArgs a3 = a;
    a3.resume = 1; a3.order = list; a3.count_dev = count; a3.queue = pb.ctr + acnqp::kPolCtrResumeQueue;
    // ... from where the first launch left them: its schedule and site-row multipliers are the warm start of pass 0 (the
    // retry passes that may follow start cold, as always).  Measured on jpl52 x 24 x 4,096, where two problems have more
    // tight rows than the polish holds: from scratch the launch took 93 ms against 61 ms without a polish.
    a3.warm_x = r->x; a3.warm_y = pb.y;
    a3.x_host = nullptr;   // (the listed problems' schedules go to the host below, whoever had the last word on them)
    a3.lb_host = nullptr; a3.ub_host = nullptr; a3.q_host = nullptr;   // (the first launch has completed the device copy)
    a3.ws_by_slot = 1; a3.grid_cap = std::min(p->batch, a.grid_oversub > 1 ? 64 : 2 * h->cus);   // (<= the grid the workspace was sized for)
    if (!a.ws_by_slot) a3.grid_cap = std::min(a3.grid_cap, a.grid_cap);
    *e = launch_solver(h, rt, a3, ws, st);
  }
  if (*e == hipSuccess && a.x_host != nullptr) {   // (not a launch of acnqp_launch_count: it belongs to this one)
    hipLaunchKernelGGL(pol_x_to_host_kernel, dim3((unsigned)std::min(p->batch, 64)), dim3(256), 0, st, list, count, p->batch,
                       h->shape.N * p->t_max, r->x, a.x_host);
    *e = hipGetLastError();
  }
  return ACNQP_OK;
}

// ---- the wide-site polish (acn_qp_polish_wide.hpp): 64 < N <= 1,024 behind the large-site kernel -------------------------
// solver kernel (unchanged; it writes x and the site-row multipliers of its best pass together, into the caller's y or a
// scratch buffer) -> list kernel (what ended MAX_ITER or SOLVED_INACCURATE: status saved, marked, listed) -> polish kernel
// over the list -> restore kernel (the saved status back where the polish gave up).  Four launches on the caller's
// stream, no host synchronisation, the last three nearly empty as a rule; cold or warm-started alike; by shape, options
// and switch, never by batch size.  It runs BEHIND the last pass, not from polish_iters on: a wide site's working set
// changes by one constraint per round, and only the ADMM's final iterate is within the 96 rounds.
int launch_wide_polish(acnqp_handle* h, acnqp_handle::Work* wk, const acnqp::Route& rt, const acnqp::TiledArgs& a, const Workspace& ws,
                       const acnqp::PolishPlan& pl, const acnqp_problems* p, const acnqp_options* o, const acnqp_results* r, hipStream_t st,
                       hipError_t* e) {
  PolishBuffers pb;
  const int rc = reserve_polish(h, wk, pl, a, p, r, st, &pb);
  if (rc != ACNQP_OK) return rc;
  int32_t* const count = pb.ctr + acnqp::kPolCtrListLength;
  acnqp::TiledArgs a1 = a;
  a1.y_out = pb.y;
  *e = launch_solver(h, rt, a1, ws, st);
  if (*e == hipSuccess) *e = acnqp::launch_polish_wide_list(r->status, pb.saved, pb.list, count, p->batch, st);
  if (*e == hipSuccess) *e = acnqp::launch_polish_wide(polish_args(h, pl, pb, p, o, r), pb.slab, pb.grid, st);
  if (*e == hipSuccess) *e = acnqp::launch_polish_wide_restore(r->status, pb.saved, pb.list, count, p->batch, st);
  return ACNQP_OK;
}

int solve_batch_device(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, acnqp_results* r, hipStream_t st, bool nothing_follows,
                       const HostTables& ht) {
  int rc = check_problem_shapes(h, p, o, r);
  if (rc != ACNQP_OK) return rc;
  if (p->batch == 0) return ACNQP_OK;
  HIP_TRY(hipSetDevice(h->device));
  acnqp::TiledArgs a = tiled_args(h, p, o, r, st);
  (void)hipGetLastError();   // drop any stale error so the checks below report this launch only
  // a problem whose workgroup never ran must not look solved (or carry the previous call's status)
  HIP_TRY(hipMemsetAsync(r->status, 0, (size_t)p->batch * sizeof(int32_t), st));
  // the launch's duration (acnqp_kernel_times, bench.py's roofline) covers everything the launch puts on the stream:
  // the two order kernels as well as the solver kernel (they used to sit in front of the start event)
  const int evk = (int)(h->launches % acnqp_handle::kEvRing);
  HIP_TRY(hipEventRecord(h->ev_start[evk], st));
  const acnqp::Route rt = route_of(h, p->t_max, p->k_sessions, p->batch);
  if (ht.x != nullptr && !rt.direct_x()) return fail(ACNQP_ERR_INVALID, "direct x on a route that cannot store it");   // (run_call asks the same table)
  if (ht.lb != nullptr && !rt.direct_in()) return fail(ACNQP_ERR_INVALID, "direct inputs on a route that cannot load them");
  a.x_host = ht.x;
  a.lb_host = ht.lb; a.ub_host = ht.ub; a.q_host = ht.q;
  acnqp_handle::Work* wk = h->work_for(st);
  if ((rc = schedule_launch(h, wk, rt, p, st, &a)) != ACNQP_OK) return rc;
  Workspace ws;
  if ((rc = reserve_workspace(wk, rt, st, &a, &ws)) != ACNQP_OK) return rc;
  // the polish: shape, switches and options decide in ONE place (acn_qp_polplan.hpp)
  const acnqp::PolishPlan pl = polish_plan_of(h, rt, o->polish_iters, o->max_iter, a.warm_x != nullptr);
  hipError_t e = hipSuccess;
  switch (pl.kind) {
    case acnqp::PolishKind::on_chip:
    case acnqp::PolishKind::long_horizon:
      if ((rc = launch_with_polish(h, wk, rt, a, ws, pl, p, o, r, st, nothing_follows, &e)) != ACNQP_OK) return rc;
      break;
    case acnqp::PolishKind::wide:   // (cold or warm-started: it starts from the launch's last iterate)
      if ((rc = launch_wide_polish(h, wk, rt, a, ws, pl, p, o, r, st, &e)) != ACNQP_OK) return rc;
      break;
    case acnqp::PolishKind::none:
      e = launch_solver(h, rt, a, ws, st);
      break;
  }
  if (e != hipSuccess) return fail(ACNQP_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  HIP_TRY(hipEventRecord(h->ev_stop[evk], st));
  if (wk->last) HIP_TRY(hipEventRecord(wk->last, st));   // what an eviction of this stream's buffers waits for
  ++h->launches;
  return ACNQP_OK;
}

}  // namespace

// (a launch on a caller's stream: nothing of this handle's follows it)
int acnqp_solve_batch_device(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, acnqp_results* r,
                             void* hip_stream) {
  return solve_batch_device(h, p, o, r, reinterpret_cast<hipStream_t>(hip_stream), true);
}

int32_t acnqp_accel_columns(acnqp_handle* h, int32_t t_max, int32_t k_sessions, int32_t precision, int32_t requested) {
  if (!h || t_max < 1 || k_sessions < 1 || requested <= 0) return 0;
  if (precision != 64) return 0;
  // (as if the batch were unbounded: ACNQP_WAVE_MIN_BATCH never lowers the answer)
  return std::min(requested, route_of(h, t_max, k_sessions, acnqp::kRouteAnyBatch).accel_cap<Kernels>());
}

static float event_pair_ms(acnqp_handle* h, long long launch) {
  const int k = (int)(launch % acnqp_handle::kEvRing);
  if (hipEventSynchronize(h->ev_stop[k]) != hipSuccess) return -1.0f;
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, h->ev_start[k], h->ev_stop[k]) != hipSuccess) return -1.0f;
  return ms;
}

int acnqp_set_long_polish(acnqp_handle* h, int32_t on) {
  if (!h) return fail(ACNQP_ERR_INVALID, "acnqp_set_long_polish: null handle");
  h->long_polish = on != 0;
  return ACNQP_OK;
}

int acnqp_set_long_vjp(acnqp_handle* h, int32_t on) {
  if (!h) return fail(ACNQP_ERR_INVALID, "acnqp_set_long_vjp: null handle");
  h->long_vjp = on != 0;
  return ACNQP_OK;
}

int acnqp_set_wide_polish(acnqp_handle* h, int32_t on) {
  if (!h) return fail(ACNQP_ERR_INVALID, "acnqp_set_wide_polish: null handle");
  h->wide_polish = on != 0;
  return ACNQP_OK;
}

int64_t acnqp_launch_count(acnqp_handle* h) { return h ? (int64_t)h->launches : 0; }
int64_t acnqp_ordered_launch_count(acnqp_handle* h) { return h ? (int64_t)h->ordered_launches : 0; }

int acnqp_polish_stats(acnqp_handle* h, int64_t* out, int32_t capacity) {
  if (!h || !out || capacity < 1) return fail(ACNQP_ERR_INVALID, "acnqp_polish_stats: null argument");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  int32_t v[16] = {0};
  HIP_TRY(hipMemcpy(v, h->pol_stats, sizeof(v), hipMemcpyDeviceToHost));
  for (int k = 0; k < capacity && k < 16; ++k) out[k] = v[k];
  return ACNQP_OK;
}

// Introspection outside include/acn_qp.h (every build): the problems that polish launches ALONGSIDE a solver launch
// (launch_with_polish) have taken since the last call; -1 without a handle or on a HIP error.  Synchronises the device.
extern "C" int64_t acnqp_debug_polish_alongside(acnqp_handle* h) {
  if (!h || hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
  int32_t v = 0;
  if (hipMemcpy(&v, h->pol_stats + 16, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemset(h->pol_stats + 16, 0, sizeof v) != hipSuccess) return -1;
  return v;
}

// Introspection outside include/acn_qp.h (every build): the problems of the handle's last host-entry call
// (acnqp_solve_batch / _batches / _table) whose schedule the kernel stored straight into the caller's result array
// (the direct path, acn_qp_pipeline.hpp) instead of a copy; 0 where every x was copied, -1 without a handle.
extern "C" int64_t acnqp_debug_direct_x(acnqp_handle* h) { return h ? (int64_t)h->direct_x_last : -1; }

// ... whose lb, ub and q the kernel loaded straight from the caller's arrays (the direct path for the inputs,
// acn_qp_pipeline.hpp) instead of a copy; 0 where every input was copied, -1 without a handle.
extern "C" int64_t acnqp_debug_direct_in(acnqp_handle* h) { return h ? (int64_t)h->direct_in_last : -1; }

// Introspection outside include/acn_qp.h (every build): out[0] = live eigenpairs of the site's G G', out[1] = the MFMA
// k-steps that hold them once compacted (acn_qp_rank.hpp), out[2] = the eigen extent in k-steps of the wave kernel's
// instantiation this handle's launches run (the full one is MR / 4).  Returns 0, -1 without a handle.
extern "C" int acnqp_debug_wave_rank(acnqp_handle* h, int32_t* out) {
  if (!h || !out) return -1;
  const int ext = wave_extent_of(h);
  out[0] = h->site.rank; out[1] = h->site.eig_ksteps; out[2] = ext > 0 ? ext : h->shape.MR / 4;
  return 0;
}

// Introspection outside include/acn_qp.h (every build): the launch-order keys (launch_order_keys: what a launch of at
// least kOrderMinBatch problems is sorted by) of the DEVICE-resident problems p, of any batch size, copied to the host
// array keys_out[p->batch].  Synchronises.  Returns 0, -1 on a null argument or a HIP error.
extern "C" int acnqp_debug_order_keys(acnqp_handle* h, const acnqp_problems* p, int32_t* keys_out) {
  if (!h || !p || !keys_out || p->batch < 0 || p->t_max < 1 || p->k_sessions < 1) return -1;
  if (p->batch == 0) return 0;
  if (!p->lb || !p->ub || !p->s_off || !p->s_len || !p->s_cap || !p->horizon) return -1;
  if (hipSetDevice(h->device) != hipSuccess) return -1;
  int32_t* keys = nullptr;
  if (hipMalloc((void**)&keys, (size_t)p->batch * sizeof(int32_t)) != hipSuccess) return -1;
  hipError_t e = launch_order_keys(h, route_of(h, p->t_max, p->k_sessions, p->batch), p, nullptr, keys);
  if (e == hipSuccess) e = hipMemcpy(keys_out, keys, (size_t)p->batch * sizeof(int32_t), hipMemcpyDeviceToHost);
  (void)hipFree(keys);
  return e == hipSuccess ? 0 : -1;
}

// Introspection outside include/acn_qp.h (every build): out[0] = the site's EVSEs, out[1] = the MFMA k-steps of P = Ghat r0
// that hold one (four EVSEs each), out[2] = the EVSE k-steps the wave kernel's instantiation for this handle runs
// (acn_qp_rank.hpp; 16 = all of them).  Returns 0, -1 without a handle.
extern "C" int acnqp_debug_wave_evse_extent(acnqp_handle* h, int32_t* out) {
  if (!h || !out) return -1;
  out[0] = h->shape.N; out[1] = (h->shape.N + 3) / 4; out[2] = wave_evse_extent_of(h);
  return 0;
}

#ifdef ACNQP_DEBUG_WS
// diagnostic builds only (tools/gpu_long_race.py): the most recently used kernel workspace, copied to the host
extern "C" int64_t acnqp_debug_copy_workspace(acnqp_handle* h, double* out, int64_t n_doubles) {
  if (!h || h->work.empty()) return -1;
  size_t best = 0;
  for (size_t k = 1; k < h->work.size(); ++k) if (h->work[k].used > h->work[best].used) best = k;
  (void)hipDeviceSynchronize();
  const int64_t have = (int64_t)(h->work[best].buf.cap / sizeof(double));
  const int64_t n = std::min(have, n_doubles);
  if (out && n > 0 && hipMemcpy(out, h->work[best].buf.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  return have;
}
#endif

float acnqp_last_kernel_ms(acnqp_handle* h) {
  if (!h || h->launches == 0) return -1.0f;
  return event_pair_ms(h, h->launches - 1);
}

int32_t acnqp_kernel_times(acnqp_handle* h, float* out_ms, int32_t capacity) {
  if (!h || !out_ms || capacity <= 0) return 0;
  long long first = std::max(h->reported, h->launches - acnqp_handle::kEvRing);
  first = std::max(first, h->launches - (long long)capacity);
  int32_t n = 0;
  for (long long l = first; l < h->launches; ++l) out_ms[n++] = event_pair_ms(h, l);
  h->reported = h->launches;
  return n;
}

namespace {

int check_table(const acnqp_handle* h, const acnqp_table* t, const acnqp_options* o, const acnqp_results* r) {
  if (!h || !t || !o || !r) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: null argument");
  if (t->batch < 0) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: negative batch");
  if (t->batch == 0) return ACNQP_OK;
  if (!t->horizon || !t->q_index || !t->q_table || !t->pdiag || !t->s_eq || !t->sess_seg || !t->rate_seg ||
      (t->n_sessions > 0 && (!t->s_evse || !t->s_slot || !t->s_off || !t->s_len || !t->s_cap)))
    return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: null table array");
  if (t->n_sessions < 0 || t->n_horizons < 1) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: bad n_sessions / n_horizons");
  // the dense view for the shared checks (pointers only tested for null there)
  static const double dummy_d = 0;
  static const int32_t dummy_i = 0;
  acnqp_problems p;
  p.batch = t->batch; p.t_max = t->t_max; p.k_sessions = t->k_sessions; p.horizon = t->horizon;
  p.lb = p.ub = p.q = p.s_cap = &dummy_d; p.pdiag = t->pdiag; p.s_off = p.s_len = &dummy_i; p.s_eq = t->s_eq;
  p.peak = t->peak; p.lf = t->lf; p.dc = t->dc; p.dfloor = t->dfloor; p.warm_x = p.warm_y = nullptr;
  const int rc = check_problem_shapes(h, &p, o, r);
  if (rc != ACNQP_OK) return rc;
  const int B = t->batch, S = t->n_sessions, N = h->shape.N, Tm = t->t_max, K = t->k_sessions;
  if (t->sess_seg[0] != 0 || t->sess_seg[B] != S) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: sess_seg must run from 0 to n_sessions");
  for (int b = 0; b < B; ++b) {
    if (t->sess_seg[b + 1] < t->sess_seg[b]) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: sess_seg is not non-decreasing");
    if (t->q_index[b] < 0 || t->q_index[b] >= t->n_horizons) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: q_index out of range");
    if (t->horizon[b] < 1 || t->horizon[b] > Tm) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: horizon out of range");
  }
  if (t->rate_seg[0] != 0) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: rate_seg must start at 0");
  for (int s_ = 0; s_ < S; ++s_) {
    const int len = t->s_len[s_] > 0 ? t->s_len[s_] : 0;
    if (t->s_evse[s_] < 0 || t->s_evse[s_] >= N || (len > 0 && (t->s_slot[s_] < 0 || t->s_slot[s_] >= K)))
      return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: session " + std::to_string(s_) + ": EVSE or slot out of range");
    if (len > 0 && (t->s_off[s_] < 0 || t->s_off[s_] + len > Tm))
      return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: session " + std::to_string(s_) + ": window outside [0, t_max)");
    if (t->rate_seg[s_ + 1] - t->rate_seg[s_] != len)
      return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: session " + std::to_string(s_) +
                                     ": min_rates / max_rates must have one entry per remaining period (aco.py:68, 73)");
  }
  if (t->rate_seg[S] > 0 && (!t->min_rates || !t->max_rates)) return fail(ACNQP_ERR_INVALID, "acnqp_solve_table: null rate arrays");
  return ACNQP_OK;
}

}  // namespace

int acnqp_solve_table(acnqp_handle* h, const acnqp_table* t, const acnqp_options* o, acnqp_results* r) {
  const auto tcheck0 = std::chrono::steady_clock::now();
  const int rc0 = check_table(h, t, o, r);
  if (rc0 != ACNQP_OK) return rc0;
  if (t->batch == 0) return ACNQP_OK;
  HIP_TRY(hipSetDevice(h->device));
  Call call;
  call.T = t; call.R = r;
  call.bs.push_back(BatchShape{t->batch, t->t_max, t->k_sessions, false, r->y != nullptr});
  const double check_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tcheck0).count();
  return solve_call(h, call, o, "acnqp_solve_table", check_ms);
}

int acnqp_solve_batches(acnqp_handle* h, int32_t n_batches, const acnqp_problems* p, const acnqp_options* o, acnqp_results* r) {
  if (!h || !p || !o || !r || n_batches < 0) return fail(ACNQP_ERR_INVALID, "acnqp_solve_batches: null argument or negative count");
  Call call;
  call.P = p; call.R = r;
  for (int g = 0; g < n_batches; ++g) {
    const int rc = check_problem_shapes(h, p + g, o, r + g);
    if (rc != ACNQP_OK) return rc;
    call.bs.push_back(BatchShape{p[g].batch, p[g].t_max, p[g].k_sessions, p[g].warm_x != nullptr, r[g].y != nullptr});
  }
  HIP_TRY(hipSetDevice(h->device));
  return solve_call(h, call, o, "acnqp_solve_batches", -1.0);
}

int acnqp_solve_batch(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, acnqp_results* r) {
  return acnqp_solve_batches(h, 1, p, o, r);
}

void* acnqp_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    g_last_error = "acnqp_host_alloc: hipHostMalloc failed";
    return nullptr;
  }
  return p;
}

void acnqp_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

}  // extern "C"
