/*
 * acn_qp.h -- C ABI of the MI355X batched MPC solver for adacharge.
 *
 * This is the drop-in boundary.  The reference has no FFI
 * at this path: its "solver call" is the Python statement
 *
 *     prob.solve(solver=self.solver, verbose=verbose)
 *         /root/reference/adacharge/adaptive_charging_optimization.py:318
 *
 * on a cvxpy Problem assembled at aco.py:220-284 and 315-317.  Each entry point
 * below names the piece of that path it replaces.  Plain C types only; every
 * buffer is owned by the caller; nothing is retained after a call returns
 * (for the *_device form: after the stream has drained).
 *
 * Problem solved, for every b in [0, batch):
 *
 *   minimise    1/2 pdiag_b |r|^2 + <q_b, r>                   r in R^{N x Tm}
 *   subject to  lb_b <= r <= ub_b                                (aco.py:61-79)
 *               sum_{t in [off, off+len)} r[i, t] <= cap          (aco.py:105-123;
 *                   (== cap when s_eq_b)                            cap in A-periods)
 *               for every period t, rows of the site matrix G:
 *                 LINEAR  (G r[:, t])_j <= limits_j               (aco.py:165-172)
 *                 SOC     |((G r)_j, (G r)_{j+M})|_2 <= limits_j  (aco.py:151-164)
 *                 peak    sum_i r[i, t] <= peak_b[t]              (aco.py:196-198)
 *   plus, when the site carries a "flat" row v = voltages / 1e3 (kW per A), the objective term
 *               1/2 lf_b sum_t (v' r[:, t])^2                     (load_flattening, aco.py:403-408;
 *                                                                  its linear part is already in q)
 *   and, when it carries a "max" row (same v), the objective term
 *               dc_b * max(max_t v' r[:, t], dfloor_b)            (demand_charge / peak, aco.py:387-400)
 *
 * Layouts are C order: r, lb, ub, q are [batch][N][Tm] -- the (N, T) rates
 * matrix the reference returns at aco.py:321, one per problem.
 */
#ifndef ACN_QP_H
#define ACN_QP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACNQP_ABI_VERSION 10

/* cone of the infrastructure rows (constraint_type at aco.py:35, 151, 165) */
#define ACNQP_CONE_LINEAR 0
#define ACNQP_CONE_SOC 1

/* per-problem status; the Python layer maps anything but SOLVED to
 * InfeasibilityException exactly as aco.py:319-320 does for cvxpy statuses */
#define ACNQP_STATUS_UNSET 0
#define ACNQP_STATUS_SOLVED 1             /* cp.OPTIMAL                     */
#define ACNQP_STATUS_MAX_ITER 2           /* residuals above tolerance at max_iter, or stalled above the
                                             SOLVED_INACCURATE level (no 10 % progress for options.stall_iters
                                             iterations), in every pass (options.retry_passes)              */
#define ACNQP_STATUS_PRIMAL_INFEASIBLE 3  /* ADMM certificate (cp.INFEASIBLE) */
#define ACNQP_STATUS_EMPTY_SET 4          /* a session's bounds cannot meet its energy row */
#define ACNQP_STATUS_SOLVED_INACCURATE 5   /* max_iter or the stall rule ended every pass short of the tolerance,
                                             the best one with both residuals within 100x their tolerance or
                                             within options.inaccurate_floor, whichever is looser:
                                             cp.OPTIMAL_INACCURATE, which the reference accepts (aco.py:319) */

/* return codes (never C++ exceptions across the ABI) */
#define ACNQP_OK 0
#define ACNQP_ERR_INVALID (-1)     /* bad argument / unsupported shape */
#define ACNQP_ERR_HIP (-2)         /* HIP runtime failure              */
#define ACNQP_ERR_NO_DEVICE (-3)

/* kernel families (acnqp_route): which kernel serves a launch is a function of the site and the padded shape */
#define ACNQP_ROUTE_WAVE1 1        /* wave per problem: one row tile, horizon <= 12, one wave             */
#define ACNQP_ROUTE_WAVE2 2        /* ... one row tile, horizon 13-24, two waves                          */
#define ACNQP_ROUTE_WAVE3 3        /* ... two row tiles, horizon <= 12, two waves of six periods           */
#define ACNQP_ROUTE_WAVE4 4        /* ... two row tiles, horizon 13-24, four waves of six periods          */
#define ACNQP_ROUTE_WAVE5 5        /* ... one row tile, horizon 33-48, four waves                          */
#define ACNQP_ROUTE_TILED_CT1 6    /* register-resident tiled kernel, one column tile (horizon <= 16)      */
#define ACNQP_ROUTE_TILED_CT2 7    /* ... two column tiles (horizon 17-32)                                 */
#define ACNQP_ROUTE_LONG_LDS 8     /* long-horizon MFMA kernel, site-row state in LDS                      */
#define ACNQP_ROUTE_LONG_WS 9      /* long-horizon MFMA kernel, state in a workspace                       */
#define ACNQP_ROUTE_STREAM 10      /* large-site MFMA kernel (N > 64, horizon <= 48)                       */
#define ACNQP_ROUTE_GENERAL 11     /* general-shape kernel                                                 */

typedef struct acnqp_handle acnqp_handle; /* opaque; one per (site, GPU) */

/* Site data shared by every problem of a batch: what InfrastructureInfo
 * contributes to aco.py:126-198.  G is [n_rows][n_evse] row-major:
 *   LINEAR: |constraint_matrix| (n_infra rows)            aco.py:171
 *   SOC:    [C*cos(phi); C*sin(phi)] (2*n_infra rows)     aco.py:156-158
 *   then one row voltages/1e3 iff has_flat               aco.py:336-344, 406
 *   then one row voltages/1e3 iff has_max                aco.py:387-400
 *   then one all-ones row iff has_peak                   aco.py:197          */
typedef struct {
  int32_t n_evse;        /* N                                   */
  int32_t n_infra;       /* M: rows of constraint_matrix         */
  int32_t n_rows;        /* rows of G = M or 2M, + has_flat + has_max + has_peak; at most 48 AFTER the
                            kernels' padding: SOC pads its 2M rows to 8*ceil(M/4), so a SOC site
                            needs 8*ceil(M/4) + has_flat + has_max + has_peak <= 48 (M <= 20 with a
                            peak, flat or max row, M <= 24 without); LINEAR: n_rows <= 48        */
  int32_t cone;          /* ACNQP_CONE_*                         */
  int32_t has_peak;      /* 0 / 1                                */
  int32_t has_flat;      /* 0 / 1: aggregate-power row for load_flattening */
  int32_t has_max;       /* 0 / 1: aggregate-power row for demand_charge / peak */
  const double* G;       /* [n_rows * n_evse]                    */
  const double* limits;  /* [n_infra]  constraint_limits         */
} acnqp_site;

/* One batch of structured problems.  Pointers are HOST pointers for
 * acnqp_solve_batch and DEVICE pointers for acnqp_solve_batch_device. */
typedef struct {
  int32_t batch;           /* B                                              */
  int32_t t_max;           /* Tm: padded horizon of every array below        */
  int32_t k_sessions;      /* K: session slots per EVSE (>= 1; disjoint windows
                              per EVSE; offline instances, adacharge.py:249-276,
                              reach tens of sessions per EVSE)                */
  const int32_t* horizon;  /* [B]        own horizon T_b <= Tm (aco.py:243)  */
  const double* lb;        /* [B*N*Tm]   0 outside session windows           */
  const double* ub;        /* [B*N*Tm]   finite                              */
  const double* q;         /* [B*N*Tm]   linear cost (minimisation form)     */
  const double* pdiag;     /* [B]        P = pdiag * I  (2 * equal_share)    */
  const int32_t* s_off;    /* [B*K*N]    window start per (slot, EVSE)       */
  const int32_t* s_len;    /* [B*K*N]    window length, 0 = empty slot       */
  const double* s_cap;     /* [B*K*N]    energy cap in A-periods             */
  const uint8_t* s_eq;     /* [B]        1: energy rows are equalities       */
  const double* peak;      /* [B*Tm] or NULL; +inf = unlimited period        */
  const double* lf;        /* [B] or NULL: weight of 1/2 lf (v' r_t)^2 (2 * load_flattening coefficient) */
  const double* dc;        /* [B] or NULL: weight (>= 0) of max(max_t v' r_t, dfloor)  [$ per kW]     */
  const double* dfloor;    /* [B] or NULL: previous / baseline peak in kW (aco.py:390-394)           */
  /* Optional warm start (both or neither; NULL = cold, which is what the reference does: nothing survives a
   * schedule() call, adacharge.py:152-158).  A closed-loop caller passes the previous step's schedule and
   * site-row multipliers (results.y), both shifted by the periods that have elapsed.  The solve then starts from
   * z = Proj(warm_x), y2 = warm_y and the multipliers of the box / energy set that make the pair stationary,
   * y1 = -(P z + q + G' y2).  The optimum does not depend on it; the iteration count does.                       */
  const double* warm_x;    /* [B*N*Tm] or NULL                                                        */
  const double* warm_y;    /* [B*n_rows*Tm] or NULL: multipliers of the rows of acnqp_site.G, per period.
                              Read as zero at t >= horizon[b], whatever is stored there (a shifted y of a longer
                              horizon may leave entries behind): y stays exactly zero at dead periods            */
} acnqp_problems;

typedef struct {
  double* x;         /* [B*N*Tm]  schedule (the feasible ADMM iterate z)      */
  int32_t* status;   /* [B]       ACNQP_STATUS_*                              */
  int32_t* iters;    /* [B]                                                   */
  double* pri_res;   /* [B]       |A r - z|_inf at exit                       */
  double* dua_res;   /* [B]       |P r + q + A'y|_inf at exit                 */
  double* obj;       /* [B]       1/2 pdiag |x|^2 + <q, x>                    */
  double* y;         /* [B*n_rows*Tm] or NULL (not wanted): multipliers of the rows of acnqp_site.G at exit
                        (row order and units of G; a SOC pair's two rows carry the pair's two components)
                        -- the warm_y of a later, similar problem                                 */
  double* x_dev;     /* host-buffer entry points only, optional (NULL = not wanted): a DEVICE
                        pointer [B*N*Tm] on the handle's GPU that also receives the schedules,
                        so that a collective (the RCCL all-gather of a multi-GPU job) can start
                        from HBM without re-uploading them.  Ignored by acnqp_solve_batch_device. */
} acnqp_results;
/* What the outputs hold for a problem that is not solved -- the same on every kernel family (tests/test_verdicts_gpu.py
 * pins it on all eleven of acnqp_route).  Every element of every output is written whatever the status.
 *   PRIMAL_INFEASIBLE, MAX_ITER:  x is the ADMM iterate z at exit: finite, lb <= x <= ub exactly, exact zeros outside
 *       the session windows and at t >= horizon[b], on the energy rows to the projection's roundoff -- a point of the
 *       box-and-energy set, NOT of the site rows, and not a schedule to apply.  y (when wanted) is the finite multiplier
 *       iterate, zero at t >= horizon[b]; obj is the objective of that x; pri_res / dua_res are the finite residuals of
 *       the last check; iters the iterations made (all passes; < max_iter for a certificate, max_iter per pass else).
 *   EMPTY_SET:  decided before any iteration, on the raw arrays (sum lb > cap, or sum ub < cap under equality, beyond
 *       64e-13 max(1, |cap|)): x = 0 and y = 0 everywhere, iters = 0, obj = 0, pri_res = dua_res = 1e300.
 * The certificate behind PRIMAL_INFEASIBLE is a test on the change v of the multipliers between two residual checks
 * (|A'v|_inf <= 1e-4 |v|_inf and a support-function bound below -1e-4 |v|_inf), not a proof: what it decides at relative
 * distances 1e-2 ... 1e-5 either side of the feasibility boundary is pinned by tests/verdict_cases.py.                 */

/* Solver options -- the knobs cvxpy would forward to its solver (the
 * reference sets none, aco.py:318; defaults: acnqp_default_options). */
typedef struct {
  double eps_abs;        /* absolute residual tolerance                       */
  double eps_rel;        /* relative residual tolerance                       */
  int32_t max_iter;
  int32_t check_every;   /* residual check period (iterations)                */
  int32_t adapt_every;   /* rho adaptation period, 0 = fixed rho              */
  double rho;            /* initial ADMM penalty                              */
  double sigma;          /* proximal weight on x                              */
  double alpha;          /* over-relaxation in (0, 2)                         */
  double adapt_tol;      /* adapt when the residual ratio leaves [1/tol, tol];
                            the band widens by tol/8 with every adaptation made,
                            so the penalty cannot cycle                          */
  double reg_rel;        /* scale-free Tikhonov floor: effective pdiag =
                            max(pdiag, reg_rel * |q|_inf / (max(ub) * T_b)); 0 disables.
                            On LP instances a small floor returns the least-norm
                            LP optimum (exact regularisation)  */
  int32_t precision;     /* 64 or 32: arithmetic type of the ADMM loop        */
  int32_t accel_mem;     /* Anderson acceleration of the ADMM fixed-point map: columns of
                            history requested (0 = plain ADMM).  The kernels use
                            min(accel_mem, what fits their LDS for the problem shape);
                            acnqp_accel_columns reports that number                */
  /* -- ABI v7 ------------------------------------------------------------------------------------------ */
  int32_t stall_iters;   /* stall rule: a pass whose residual score max(pri / eps_pri, dua / eps_dua) has not
                            improved by 10 % for this many iterations, and sits within 1.25x of its best, ends
                            (SOLVED_INACCURATE if it qualifies, MAX_ITER otherwise) instead of burning max_iter
                            iterations on a plateau.  0 = off.  Default 3000 (the longest wait between two
                            improvements seen on any converging instance of tools/ and tests/ is 1,240)     */
  int32_t retry_passes;  /* a problem whose pass ends MAX_ITER / SOLVED_INACCURATE after >= stall_iters (3000 if
                            the stall rule is off) iterations is solved again from a COLD start with a FIXED
                            penalty retry_rho * 4^(pass - 1) -- inside the same kernel launch, for every entry
                            point -- up to this many times; the best pass is returned (SOLVED > SOLVED_INACCURATE
                            > MAX_ITER, the first of equals), iters is the total.  0 = single pass.  Default 2.
                            Only when adapt_every > 0 (a caller who fixed the penalty gets that penalty only).
                            Why it works: DESIGN.md section 2 (the plateau is the adaptive penalty's doing)  */
  int32_t retry_max_iter;/* iteration limit of a retry pass (min with max_iter).  Default 8000            */
  /* -- ABI v8 ------------------------------------------------------------------------------------------ */
  int32_t polish_iters;  /* a problem of a small site (N <= 64, horizon <= 32, <= 4 sessions per EVSE, no load-flattening /
                            demand-charge row, cold start) that has not converged after this many ADMM iterations is
                            handed to the POLISH: an active-set Newton method on the KKT conditions that starts from the
                            working set the ADMM iterate suggests (variables on a bound, tight energy rows, site rows with a
                            non-zero multiplier) -- a few dozen small dense solves in one workgroup, inside the same call.
                            Its answer is accepted only with the KKT conditions verified on the full problem (status
                            SOLVED, residuals of that check in pri_res / dua_res, iters = ADMM iterations + Newton
                            rounds); otherwise the problem is solved as if there were no polish (from scratch, with the
                            retry passes).  What an interior-point method -- the reference's ECOS, aco.py:318 -- gives
                            for free: no plateau on the congested, tangentially degenerate instances.  0 = off.
                            Default 800                                                                      */
  double retry_rho;      /* penalty of the first retry pass.  Default 0.5                                 */
  double inaccurate_floor; /* residual tolerance (absolute and relative) below which a pass that ran out of
                            iterations still counts as SOLVED_INACCURATE even when 100x the requested tolerance
                            is tighter.  Default 1e-5 (what cvxpy hands OSQP as eps_abs = eps_rel).  0 = the
                            100x rule alone                                                               */
  /* -- ABI v9 ------------------------------------------------------------------------------------------ */
  int32_t polish_stall;  /* early hand-over to the polish (one-wave-per-problem kernel: N <= 64, horizon <= 12 with up to 16
                            site rows): from polish_iters / 2 on, a problem whose residual score has not improved by 10 % for
                            this many iterations goes to the polish at once instead of at polish_iters.  For a launch in
                            which every problem has a wavefront of its own -- up to 1,024 per GPU: the scenario MPC of
                            BASELINE configs[3] -- the launch lasts as long as its slowest problem, and 100 takes a
                            quarter off it (1,024 scenarios of one site: 3.4 -> 2.5 ms, 9.8 -> 7.3 ms).  On a
                            throughput-bound launch it sends ten times as many problems to the polish, most of which
                            the ADMM would have finished by itself: slower (one 256-batch per call 81 -> 62 k QP/s).
                            Same optimum either way (the polish verifies the KKT conditions).  0 = off.  Default 0 */
} acnqp_options;

/* acnqp_create -- uploads the site once.  Replaces the per-call rebuilding of
 * the infrastructure atoms at aco.py:157-172 (the reference re-creates them on
 * every MPC step, adacharge.py:152-158).  device_id: HIP ordinal. */
int acnqp_create(const acnqp_site* site, int32_t device_id, acnqp_handle** out);

/* acnqp_solve_batch -- host buffers in, host buffers out, synchronous.
 * Replaces cp.Problem(...).solve(...) at aco.py:315-318 for B problems.
 * Same as acnqp_solve_batches with one batch: a large batch is cut into chunks whose
 * H2D copies, kernels and D2H copies overlap.                                       */
int acnqp_solve_batch(acnqp_handle* h, const acnqp_problems* p,
                      const acnqp_options* o, acnqp_results* r);

/* acnqp_solve_batches -- n_batches independent host-buffer batches (p[g] -> r[g]) in
 * ONE pipelined pass, synchronous.  What a caller with many batches of MPC snapshots
 * (timesteps, sites, demand scenarios: the reference would loop over aco.py:286-321)
 * submits at once: consecutive batches of one shape (t_max, k_sessions) share kernel
 * launches of a few thousand problems, so that a launch does not idle on its slowest
 * problem; chunks rotate over internal streams with their own device staging, so that
 * the H2D copies of chunk c+1 and the D2H copies of chunk c-1 overlap chunk c's kernel.
 * Buffers allocated with acnqp_host_alloc (pinned) are copied by DMA without a staging
 * hop; pageable buffers work, slower.  A pinned r[g].x may be written by the kernels
 * themselves while the call runs (it is the call's to write until it returns; read it
 * after that).  Every pointer is a HOST pointer; nothing is
 * retained after return.  Every problem's status is set (never ACNQP_STATUS_UNSET) or
 * the call fails with ACNQP_ERR_HIP.                                                 */
int acnqp_solve_batches(acnqp_handle* h, int32_t n_batches, const acnqp_problems* p,
                        const acnqp_options* o, acnqp_results* r);

/* A batch of problems as the SESSION TABLE the reference's statement is made of, instead of the dense arrays of
 * acnqp_problems: what charging_rate_bounds (aco.py:45-79) and energy_constraints (aco.py:81-124) loop over -- one
 * record per active session -- plus the linear cost once per distinct horizon (build_objective, aco.py:200-218: it
 * depends on a problem only through T = max(offset + remaining), aco.py:243-245).  The library forms lb, ub, q and
 * the per-EVSE session slots ON THE DEVICE (acn_qp_api.hip: table_expand_*), so that a problem costs ~1-4 KB of
 * host-to-device traffic instead of 21.6 KB at 54 x 12 and no caller ever fills an (N, T) array per problem.
 * Sessions are grouped by problem: problem b owns the sessions [sess_seg[b], sess_seg[b + 1]); session s owns the
 * rate entries [rate_seg[s], rate_seg[s + 1]) -- exactly s_len[s] of them (aco.py:68, 73).  Windows of one EVSE must
 * be disjoint (s_slot numbers them 0 .. k_sessions - 1 per EVSE and problem).  All pointers are HOST pointers.      */
typedef struct {
  int32_t batch;            /* B                                                                       */
  int32_t t_max;            /* Tm >= every horizon                                                     */
  int32_t k_sessions;       /* K: session slots per EVSE                                               */
  int32_t n_sessions;       /* S                                                                       */
  int32_t n_horizons;       /* H: rows of q_table                                                      */
  const int32_t* horizon;   /* [B]       T_b                                                           */
  const int32_t* q_index;   /* [B]       row of q_table holding this problem's linear cost             */
  const double* q_table;    /* [H*N*Tm]  linear cost (minimisation form) per distinct horizon          */
  const double* pdiag;      /* [B]                                                                     */
  const uint8_t* s_eq;      /* [B]                                                                     */
  const double* peak;       /* [B*Tm] or NULL                                                          */
  const double* lf;         /* [B] or NULL                                                             */
  const double* dc;         /* [B] or NULL                                                             */
  const double* dfloor;     /* [B] or NULL                                                             */
  const int32_t* sess_seg;  /* [B+1]     sessions of problem b: [sess_seg[b], sess_seg[b+1])           */
  const int32_t* s_evse;    /* [S]       EVSE index                                                    */
  const int32_t* s_slot;    /* [S]       slot of the session among its EVSE's sessions (0 .. K-1)      */
  const int32_t* s_off;     /* [S]       arrival_offset                                                */
  const int32_t* s_len;     /* [S]       remaining_time (<= 0: no window, no energy row)               */
  const double* s_cap;      /* [S]       remaining_demand in A-periods (aco.py:114)                    */
  const int32_t* rate_seg;  /* [S+1]     rate entries of session s: [rate_seg[s], rate_seg[s+1])       */
  const double* min_rates;  /* [rate_seg[S]]  aco.py:68                                                */
  const double* max_rates;  /* [rate_seg[S]]  aco.py:73 (ub < lb -> lb, aco.py:75, is applied here)     */
} acnqp_table;

/* acnqp_solve_table -- acnqp_solve_batch for a session table: same pipeline (chunks over internal streams, copies
 * overlapped with kernels), same kernels, same results bit for bit as the dense arrays the table stands for
 * (tests/test_table_entry.py).  Cold start only; results as acnqp_solve_batch (r->y and r->x_dev honoured).        */
int acnqp_solve_table(acnqp_handle* h, const acnqp_table* t, const acnqp_options* o, acnqp_results* r);

/* Pinned (page-locked) host memory for problem / result arrays; NULL on failure.    */
void* acnqp_host_alloc(size_t bytes);
void acnqp_host_free(void* p);

/* acnqp_solve_batch_device -- same, but every pointer in *p and *r is a device
 * pointer on the handle's GPU and the work is enqueued on `hip_stream`
 * (a hipStream_t, NULL = default stream); returns without synchronising.
 * r->status is cleared to ACNQP_STATUS_UNSET on the stream before the launch: a
 * problem still UNSET after synchronisation was never processed.              */
int acnqp_solve_batch_device(acnqp_handle* h, const acnqp_problems* p,
                             const acnqp_options* o, acnqp_results* r,
                             void* hip_stream);

/* acnqp_destroy -- frees device copies of the site and the staging workspace. */
void acnqp_destroy(acnqp_handle* h);

void acnqp_default_options(acnqp_options* o);

/* Text of the last error on the calling thread ("" if none). */
const char* acnqp_last_error(void);

int32_t acnqp_abi_version(void);

/* Duration in milliseconds of the most recent kernel launched through this
 * handle, measured with HIP events on the launch stream (valid after the
 * stream has been synchronised); < 0 if none.  Used by bench.py's roofline. */
float acnqp_last_kernel_ms(acnqp_handle* h);

/* Durations (ms, oldest first) of the launches made through this handle since
 * the previous call -- at most the 64 most recent and at most `capacity` --
 * without forcing the caller to synchronise between launches (batches kept in
 * flight on several streams).  Blocks until those launches have finished.
 * Returns the number of values written.                                      */
int32_t acnqp_kernel_times(acnqp_handle* h, float* out_ms, int32_t capacity);

/* Kernel launches made through this handle since it was created (acnqp_kernel_times keeps the 64 most recent
 * durations: a caller that sums them can tell from this count whether any were dropped).                    */
int64_t acnqp_launch_count(acnqp_handle* h);

/* Of those, the launches whose QUEUE ORDER was sorted (longest expected problem first, by how much of the greedy
 * schedule the site rows reject -- ACNQP_ORDER_KEY=sessions in the environment: by session count; launches of
 * >= 768 problems on sites without a load-flattening / demand-charge row).  Test plumbing: lets a test assert that the
 * ordered path really ran.  Every launch hands its problems to the resident workgroups through a work queue (one
 * atomic counter per launch); ACNQP_NO_QUEUE=1 / ACNQP_NO_ORDER=1 in the environment select the static schedule / the
 * natural order (diagnostics: results do not depend on either).                                                    */
int64_t acnqp_ordered_launch_count(acnqp_handle* h);

/* Counters of the polish over the handle's life (synchronises the device): out[0] problems handed to the polish,
 * out[1] solved by it, out[2..5] given up because of: more tight site rows than its LDS holds, a non-positive pivot,
 * the round limit, the final KKT check; out[6] Newton rounds made; out[8..15] time per phase of the polish kernel in
 * 10 ns ticks, summed over its workgroups (rows + gradient, Schur matrix, Cholesky, triangular solves, step, ratio test,
 * update, multiplier check + verification).  Returns ACNQP_OK.  Bench / test plumbing.                               */
int acnqp_polish_stats(acnqp_handle* h, int64_t* out, int32_t capacity);

/* Anderson columns the kernels will actually use for problems of this shape
 * (t_max periods, k_sessions slots) at the given precision when `requested`
 * columns are asked for: a function of the shape only, never of the batch
 * size (the long-horizon, large-site and general-shape kernels keep their
 * ring in global memory: 5).  No reference equivalent:
 * test/bench plumbing so that a CPU restatement can run the same algorithm.  */
int32_t acnqp_accel_columns(acnqp_handle* h, int32_t t_max, int32_t k_sessions, int32_t precision,
                            int32_t requested);

/* ABI v10: the kernel family (ACNQP_ROUTE_*) a launch of `batch` problems of this padded shape (t_max periods,
 * k_sessions slots) runs on this handle's site, and in *polish (may be NULL) 1 if that launch runs the polish phase
 * under acnqp_default_options, else 0.  The library's own routing rule, read only: no device work.  Returns 0 for
 * a null handle or a shape acnqp_solve_batch refuses.  Test plumbing: lets a test assert which kernel it exercises. */
int32_t acnqp_route(acnqp_handle* h, int32_t t_max, int32_t k_sessions, int32_t batch, int32_t* polish);

/* Additive to ABI v10 (a new symbol; no structure changes): the polish for horizons 33 ... 288 on sites of up to 64 EVSEs
 * (at most four session slots, no load-flattening or demand-charge row, behind ACNQP_ROUTE_WAVE5 and ACNQP_ROUTE_LONG_WS).
 * A property of the handle, OFF after acnqp_create: with it off every launch does what it did before there was such a
 * polish.  on != 0: a cold-started launch of such a shape with 0 < options.polish_iters < options.max_iter hands the
 * problems that have not converged after polish_iters iterations to the long-horizon polish kernel, and acnqp_route
 * reports polish = 1 for the shape.  Read on the host when a launch is planned; the decision is a function of the shape,
 * the options and this switch, never of the batch size.  Returns ACNQP_OK, ACNQP_ERR_INVALID for a null handle.      */
int acnqp_set_long_polish(acnqp_handle* h, int32_t on);

/* Additive to ABI v10 (a new symbol; no structure changes): the polish for sites of 65 ... 1,024 EVSEs at horizons <= 48
 * (ACNQP_ROUTE_STREAM; at most four session slots and 8 ceil(N k_sessions / 8) <= 1,024 session columns, at most 48 rows
 * of acnqp_site.G, no load-flattening or demand-charge row).  A property of the handle, OFF after acnqp_create: with it
 * off every launch does what it did before there was such a polish.  on != 0: a launch of such a shape with
 * options.polish_iters > 0, cold or warm-started, is followed on the same stream by the wide-site polish kernel over the
 * problems the solver kernel ended ACNQP_MAX_ITER or ACNQP_SOLVED_INACCURATE, from the schedule and multipliers it wrote
 * for them: a problem the polish solves ends ACNQP_SOLVED with iters = the solver's iterations plus the Newton rounds and
 * the final check's residuals in pri_res / dua_res; one it gives up keeps every result the solver gave it.  acnqp_route
 * reports polish = 1 for the shape.  Read on the host when a launch is planned; the decision is a function of the shape,
 * the options and this switch, never of the batch size.  Returns ACNQP_OK, ACNQP_ERR_INVALID for a null handle.      */
int acnqp_set_wide_polish(acnqp_handle* h, int32_t on);

/* ---- dual report (additive to ABI v10: new symbols only, no existing structure changes) -------------------------------
 * For any answer (x, y) of the library: the multipliers of the energy rows and of the rate bounds, and the KKT
 * residuals of the full primal-dual point, computed on the GPU by one kernel that is independent of the solver loop.
 * With pd_eff the diagonal the kernels use (options.reg_rel: the Tikhonov floor of LP-like problems included -- the
 * duals are those of the problem the kernels solve), in the minimisation form and the units of this header:
 *
 *     g    = pd_eff x + q + G'y                                         [N][Tm]
 *     v    = x - g
 *     mu_s = the shift for which sum_{t in window s} clip(v - mu_s, lb, ub) = cap_s  (inequality rows: 0 when
 *            sum clip(v, lb, ub) <= cap_s, else the shift > 0) -- the multiplier of the session's energy row
 *     z    = -(g + mu_s) inside a window, 0 outside                     (> 0: multiplier of ub, < 0: of lb)
 *
 * Where the admissible shifts form an interval (every entry of the window on a bound) the value of least magnitude is
 * reported.  res holds four doubles per problem:
 *   [0] stat    |x - clip(v - mu, lb, ub)|_inf, the natural residual (amperes; zero exactly at a KKT point)
 *   [1] energy  worst energy-row violation / max(1, |cap|)
 *   [2] site    worst site-row violation / max(1, limit)   (LINEAR rows, SOC pairs, finite peak periods)
 *   [3] comp    worst multiplier x slack / (max(1, |q|_inf) max(1, limit)) over those rows, and over the demand-charge
 *               row y_t (max_t v'x_t - v'x_t) / (max(1, |q|_inf) max(1, |max_t v'x_t|))
 * Periods t >= horizon[b] and entries outside every window get exact zeros in z; an empty slot gets 0 in mu.  A problem
 * whose status is neither SOLVED nor SOLVED_INACCURATE gets zeros in mu and z and +inf in its four residuals.
 * No floating-point atomics, fixed summation order: the same problem gives the same bits in any batch, at any position. */
typedef struct {
  double* mu;   /* [B*K*N]   layout of s_cap: multiplier of each session's energy row (per A-period) */
  double* z;    /* [B*N*Tm]  or NULL (not wanted): multipliers of the rate bounds                     */
  double* res;  /* [B*4]     stat, energy, site, comp                                                */
} acnqp_duals;

/* acnqp_duals_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns without
 * synchronising.  p: the problems (warm_x / warm_y ignored); o: read for reg_rel only; x [B*N*Tm], y [B*n_rows*Tm]
 * (may be NULL for a site without rows) and status [B] (NULL: every problem counts as solved) as a solve wrote them.
 * Bad arguments, a null handle included, return ACNQP_ERR_INVALID with acnqp_last_error set.                        */
int acnqp_duals_device(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, const double* x,
                       const double* y, const int32_t* status, acnqp_duals* out, void* hip_stream);

/* acnqp_duals_host -- the same with host pointers, synchronous; a large batch is processed in chunks.  Same bits as
 * the device entry.                                                                                                  */
int acnqp_duals_host(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, const double* x,
                     const double* y, const int32_t* status, acnqp_duals* out);

/* ---- pilot signals (additive to ABI v10: new symbols only) -----------------------------------------------------------
 * What the reference does to a solved schedule before it goes to the chargers (ada.py:176-189), for a whole batch:
 *   CONTINUOUS  max(min(x, max_pilot_i), 0)
 *   DISCRETE    max(floor_to_set(x, levels_i, eps = 0.05), 0) on every entry, padding periods included; floor_to_set is
 *               the level pos - 1 with pos = #{k : levels_i[k] < x + 0.05} (the first level for pos = 0)
 *   REALLOCATE  DISCRETE, then the round robin of post.py:189-258 on period 0 of every problem: with peak the sum of the
 *               solved period 0, the sessions of the problem are visited cyclically in the stable order of the rounding
 *               loss -(x - rounded) of their EVSE (an EVSE with two sessions is visited twice per cycle); a visit of an
 *               active EVSE retires it when its pilot has reached its cap, else tries its next larger level (clipped at
 *               the last finite one) and keeps it iff  sum_i trial_i <= peak,  next <= cap  and, for every row j,
 *               re_j^2 + im_j^2 <= (limits_j + 1e-7)^2  with re_j = sum_i cre[j][i] trial_i (im_j likewise); a refused
 *               trial retires the EVSE.  An EVSE is active, with cap s_cap[s], when a session s with s_arrived[s] sits
 *               on it (the last such session counts).
 * Every sum runs over the EVSEs in increasing order, every product and every sum rounded once (no fused multiply-add,
 * no square root): tests/pilots_spec.py states the three modes in plain loops and the library returns its bits.  No
 * atomics; a problem gives the same bits alone and at any position of any batch.  A problem makes at most
 * n_evse * n_levels visits of an active EVSE; one that is still active then (an EVSE whose last level lies below its cap:
 * the reference never returns on it) ends there with visits = -1.                                                      */
#define ACNQP_PILOTS_CONTINUOUS 0
#define ACNQP_PILOTS_DISCRETE 1
#define ACNQP_PILOTS_REALLOCATE 2

typedef struct {
  int32_t batch, t_max, n_evse, n_infra, n_levels, n_sessions;
  int32_t mode;               /* ACNQP_PILOTS_*                                                                    */
  const double* cre;          /* [M*N] real part of the infrastructure rows: constraint_matrix * cos(phase)        */
  const double* cim;          /* [M*N] imaginary part; both in the SOC form whatever the handle's cone, because
                                 the reference's feasibility test (utils.py:5-12) always uses it                   */
  const double* limits;       /* [M]                                                                                */
  const double* max_pilot;    /* [N]   CONTINUOUS only                                                              */
  const double* levels;       /* [N*L] allowable pilots per EVSE, ascending, padded with +inf (DISCRETE, REALLOCATE) */
  const int32_t* sess_seg;    /* [B+1] problem b owns the sessions [sess_seg[b], sess_seg[b+1])   (REALLOCATE)      */
  const int32_t* s_evse;      /* [S]   EVSE of the session; the order inside a problem breaks ties of the loss      */
  const uint8_t* s_arrived;   /* [S]   1: arrival_offset == 0 and a non-empty window                                */
  const double* s_cap;        /* [S]   min(remaining amp-periods, max_rates[0], max_pilot) of an arrived session    */
} acnqp_pilot_plan;

typedef struct {
  double* pilots;    /* [B*N*Tm] or NULL                                                                            */
  double* first;     /* [B*N]    or NULL: period 0 only (what goes to the chargers)                                 */
  int32_t* visits;   /* [B]      or NULL: visits of an active EVSE the round robin made (0 in the other modes),
                                 -1: stopped at the bound                                                           */
} acnqp_pilots;

/* acnqp_pilots_device -- every pointer in *plan and *out and x [B*N*Tm] is a device pointer on the handle's GPU;
 * enqueued on `hip_stream`, returns without synchronising.  At least one of out->pilots / out->first is wanted, and no
 * output may alias x.  A null handle, n_evse other than the handle's, a mode out of range or no output return
 * ACNQP_ERR_INVALID with acnqp_last_error set, before any device work.                                              */
int acnqp_pilots_device(acnqp_handle* h, const acnqp_pilot_plan* plan, const double* x, acnqp_pilots* out,
                        void* hip_stream);

/* acnqp_pilots_host -- the same with host pointers, synchronous; a large batch is processed in chunks.  Same bits as
 * the device entry.                                                                                                  */
int acnqp_pilots_host(acnqp_handle* h, const acnqp_pilot_plan* plan, const double* x, acnqp_pilots* out);

/* ---- time passes (additive to ABI v10: new symbols only) --------------------------------------------------------------
 * The fourth link of a closed MPC loop.  Every period the reference's users solve, send the first-period pilots to the
 * chargers, integrate the delivered energy and build the next problem (aco.py:45-124, 200-245 on new SessionInfo lists).
 * This entry does the last two for a whole batch: the problems `cur` just solved and the pilots `applied` in period 0
 * in, the problems of the next period out, so that the state of a batch of simulations never leaves the GPU.  For
 * every problem b, in this order (primes mark the output):
 *    1  a_i = applied[b][i] if status is NULL or status[b] is SOLVED or SOLVED_INACCURATE, else a_i = 0: time passes and
 *       nothing is delivered.
 *    2  every slot (k, i) with s_len > 0:  if s_off > 0, off' = off - 1;  otherwise len' = len - 1 and
 *       cap' = cap - a_i (one subtraction), then cap' = 0 if cap' < 0.  The slot is retired when len' == 0 or
 *       cap' <= done_tol; a retired or empty slot gets off' = len' = 0 and cap' = 0.  (A slot whose window does not lie
 *       inside [0, t_max) is no state of this shape: it is retired unread, with flag bit 4.)
 *    3  lb'[i][t] = lb[i][t + 1] for t < t_max - 1 and 0 at t_max - 1; ub' likewise; both are then set to 0 on the
 *       shifted window [off', off' + len') of every slot retired in rule 2.
 *    4  the arrivals of b -- the records [a_seg[b], a_seg[b + 1]), each with offset 0 -- are admitted in record order,
 *       serially per EVSE.  A record is refused with flag bit 1, and ignored, if its EVSE or slot is out of range, if
 *       a_len < 1 or a_len > t_max, if its rate entries [a_rate_seg[r], a_rate_seg[r] + a_len) leave the rate arrays, if
 *       its slot is live, or if [0, a_len) meets a live window of that EVSE.  Otherwise the slot becomes
 *       (0, a_len, a_cap), lb'[i][0 : a_len] = a_min and ub'[i][0 : a_len] = (a_max < a_min ? a_min : a_max) (aco.py:75).
 *    5  horizon' = max(1, max over the live slots of off' + len').
 *    6  q'[b] = q_table[h_row[horizon']] and pdiag', lf', dc' = h_scal[h_row[horizon']]; a row outside [0, n_horizons)
 *       sets flag bit 2 and writes q' and the three scalars as zeros.
 *   6b  with a clock cost (acnqp_advance_priced_device / _host), where the horizon has a row:
 *       q'[i][t] = q_table[row][i][t] + coef * (weight[i] * series[b][step + 1 + t]) for t < horizon' -- a product, a
 *       product and a sum, each rounded once, in this order; for t >= horizon' q' stays the table's entry (its zero
 *       padding), and without a row (flag bit 2) q' stays all zeros.  This is the builder's q of an objective whose LAST
 *       component is coef * tou_energy_cost, bit for bit: -(S + coef * ((-w) * price)) = -S + coef * (w * price).
 *    7  peak'[t] = peak_series[b][step + 1 + t] for t < horizon' and +inf beyond (the builder's padding); all +inf when
 *       peak_series is NULL.
 *    8  dfloor' = max(dfloor, kw_per_amp * sum_i a_i): the sum in increasing i, every operation rounded once.
 *    9  when wanted, warm_x'[i][t] = x[i][t + 1] and warm_y'[j][t] = y[j][t + 1] for t + 1 < t_max, 0 at the last period.
 *       With warm_arrival_gain g != 0, warm_x' of a session admitted in rule 4 is (-g) * q'[i][t] on its window [0, a_len)
 *       instead (one product; q' is the final one, after rule 6b): the point a cold solve starts that session from,
 *       before its projection on the bounds and the energy row (the solver kernels use g = 1e5).  0 leaves the shifted
 *       x, which is 0 for an EVSE that was idle.
 *   10  flags[b] is written for every problem, 0 when nothing was refused.
 * s_eq does not change with time and is not written.  Copies, comparisons, one subtraction per served slot and one
 * ordered sum per problem: tests/advance_spec.py states the rules in plain loops and the library returns its bits.  No
 * atomics; every output element is written whatever the input; a problem gives the same bits alone and at any position
 * of any batch.  step = -1 on an empty state (every s_len 0, applied 0) builds the first period's problems from their
 * arrivals.                                                                                                            */
#define ACNQP_ADVANCE_REFUSED 1   /* flags: an arrival record was refused (rule 4)                  */
#define ACNQP_ADVANCE_NO_ROW 2    /* flags: no objective row for the new horizon (rule 6)           */
#define ACNQP_ADVANCE_BAD_SLOT 4  /* flags: a slot of the current state lay outside [0, t_max)      */

typedef struct {
  int32_t n_evse;             /* N: must be the handle's                                                              */
  int32_t n_rows;             /* rows of the handle's G (the rows of y)                                               */
  int32_t n_horizons;         /* H: rows of q_table and h_scal                                                       */
  int32_t step;               /* the period just completed (>= -1): rule 7 reads peak_series from step + 1           */
  int32_t peak_len;           /* P >= step + 1 + t_max when peak_series is given                                      */
  int32_t n_arrivals;         /* A: arrival records                                                                   */
  int32_t n_rates;            /* R: entries of a_min / a_max                                                          */
  double done_tol;            /* a slot with cap' <= done_tol is done (A-periods)                                     */
  double kw_per_amp;          /* rule 8                                                                               */
  double warm_arrival_gain;   /* rule 9; 0 = off                                                                      */
  const double* q_table;      /* [H*N*Tm] linear cost per horizon (what objective_terms returns, zero-padded to Tm)   */
  const double* h_scal;       /* [H*3]    pdiag, lf, dc per horizon                                                   */
  const int32_t* h_row;       /* [Tm+1]   row of q_table / h_scal for a horizon, -1: none                            */
  const double* peak_series;  /* [B*P] or NULL (a site without a peak row, or no limit)                              */
  const int32_t* a_seg;       /* [B+1]    arrivals of problem b: [a_seg[b], a_seg[b+1]); NULL iff A == 0              */
  const int32_t* a_evse;      /* [A]      the session records of acnqp_table, every offset 0                         */
  const int32_t* a_slot;      /* [A]                                                                                  */
  const int32_t* a_len;       /* [A]                                                                                  */
  const double* a_cap;        /* [A]      A-periods                                                                   */
  const int32_t* a_rate_seg;  /* [A+1]    rate entries of record r start at a_rate_seg[r]                             */
  const double* a_min;        /* [R]                                                                                  */
  const double* a_max;        /* [R]                                                                                  */
} acnqp_advance_plan;

/* The next period's problems: the arrays of acnqp_problems, writable.  None may alias its source in `cur` (or x, y). */
typedef struct {
  int32_t* horizon;  /* [B]                                                  */
  double* lb;        /* [B*N*Tm]                                             */
  double* ub;        /* [B*N*Tm]                                             */
  double* q;         /* [B*N*Tm]                                             */
  double* pdiag;     /* [B]                                                  */
  int32_t* s_off;    /* [B*K*N]                                              */
  int32_t* s_len;    /* [B*K*N]                                              */
  double* s_cap;     /* [B*K*N]                                              */
  double* peak;      /* [B*Tm]; required iff the site has a peak row         */
  double* lf;        /* [B];    required iff the site has a flat row         */
  double* dc;        /* [B];    required iff the site has a max row          */
  double* dfloor;    /* [B];    required iff the site has a max row          */
  double* warm_x;    /* [B*N*Tm] or NULL (not wanted)                        */
  double* warm_y;    /* [B*n_rows*Tm] or NULL (not wanted)                   */
} acnqp_next;

/* acnqp_advance_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns
 * without synchronising.  cur: batch, t_max, k_sessions and lb, ub, s_off, s_len, s_cap (dfloor on a site with a max
 * row) are read; applied [B*N]; status [B] or NULL; x [B*N*Tm] and y [B*n_rows*Tm] are read only for next->warm_x /
 * next->warm_y.  A null handle or argument, n_evse or n_rows other than the handle's, a site row without its array, a
 * shape out of range, step < -1, a peak_len below step + 1 + t_max, or an output that overlaps an input or another
 * output return ACNQP_ERR_INVALID with acnqp_last_error set, before any device work.                                 */
int acnqp_advance_device(acnqp_handle* h, const acnqp_problems* cur, const double* applied, const int32_t* status,
                         const double* x, const double* y, const acnqp_advance_plan* plan, acnqp_next* next,
                         int32_t* flags, void* hip_stream);

/* acnqp_advance_host -- the same with host pointers, synchronous; a large batch is processed in chunks.  Same bits as
 * the device entry.                                                                                                  */
int acnqp_advance_host(acnqp_handle* h, const acnqp_problems* cur, const double* applied, const int32_t* status,
                       const double* x, const double* y, const acnqp_advance_plan* plan, acnqp_next* next,
                       int32_t* flags);

/* The clock cost of rule 6b (additive to ABI v10: new symbols only): a linear cost that follows the clock, such as a
 * time-of-use tariff -- coef * weight[i] * series[b][absolute period] per ampere of EVSE i.                           */
typedef struct {
  int32_t n_evse;        /* N: must be the handle's                                                                   */
  int32_t series_len;    /* P >= step + 1 + t_max                                                                     */
  double coef;           /* finite                                                                                    */
  const double* weight;  /* [N]                                                                                       */
  const double* series;  /* [B*P] series[b][p]: period p counted from the run's first period (step + 1 = 0)          */
} acnqp_clock_cost;

/* acnqp_advance_priced_device / _host -- acnqp_advance_device / _host with rule 6b.  cost == NULL is exactly the plain
 * entry (which is this call with NULL).  With a cost, additionally refused with ACNQP_ERR_INVALID and acnqp_last_error
 * set, before any device work: n_evse other than the handle's, a null weight or series, a coef that is not finite,
 * series_len < step + 1 + t_max, a weight or series span that meets an output of `next` or `flags`.  The host entry
 * stages `series` per problem (as peak_series) and `weight` once per call; same bits as the device entry, at any
 * chunking.                                                                                                          */
int acnqp_advance_priced_device(acnqp_handle* h, const acnqp_problems* cur, const double* applied, const int32_t* status,
                                const double* x, const double* y, const acnqp_advance_plan* plan,
                                const acnqp_clock_cost* cost, acnqp_next* next, int32_t* flags, void* hip_stream);
int acnqp_advance_priced_host(acnqp_handle* h, const acnqp_problems* cur, const double* applied, const int32_t* status,
                              const double* x, const double* y, const acnqp_advance_plan* plan,
                              const acnqp_clock_cost* cost, acnqp_next* next, int32_t* flags);

/* The adjoint of time passes (additive to ABI v10: new symbols only, no new struct) -- one call of the backward sweep
 * through a closed loop solve -> continuous pilots -> advance.  L is a scalar of the pilots `applied` of every step, as
 * the advance saw them.  The call for step s (plan->step = s, plan->a_seg the row the forward advance after period s
 * took) reads the state of step s in `cur` (s_off, s_len, s_cap), applied [B*N], status [B] or NULL, the step's
 * schedules x [B*N*Tm], max_pilot [N] of the continuous pilot rule, gdir [B*N] = dL/d applied of step s, and the adjoints
 * of the state of step s + 1: gq_next [B*N*Tm] and gcap_vjp_next [B*K*N] (gq and gcap of that step's acnqp_vjp_device),
 * gcap_carry_next [B*K*N] (gcap_carry of the previous call of this entry), horizon_next [B] (that state's horizon) and
 * flags_next [B] (the flags of the advance that built it).  Each of the five may be NULL and then counts as zeros: the
 * last step of a run has no next state.  For every problem b:
 *   A1  G[k][i] = gcap_vjp_next[k][i] + gcap_carry_next[k][i], one addition: dL/d(s_cap) of the next state.
 *   A2  with a clock cost, gprice and gq_next, where flags_next has no bit 2: for t < horizon_next,
 *       gprice[b][step + 1 + t] += coef * (sum over i, increasing, of weight[i] * gq_next[i][t]) -- rule 6b's adjoint.
 *       gprice [B*series_len] is accumulated over the calls of a sweep: the caller zeroes it once.
 *   A3  rules 1, 2 and 4 are replayed on `cur` with the forward's comparisons: which slots are kept, which of those
 *       were served (s_off == 0), which arrival records were admitted and into which slot.
 *   A4  gcap_carry[k][i] = G[k][i] for a kept slot, exact 0 for any other.
 *   A5  ga[i] = gdir[i], then minus G[k][i] for k ascending over the kept, served slots; exact 0 for a problem whose
 *       status rule 1 does not serve.
 *   A6  gx[i][0] = ga[i] where 0 <= x[i][0] <= max_pilot[i] (the clip is inactive), exact 0 elsewhere and for t >= 1:
 *       the gx of acnqp_vjp_device for step s.
 *   A7  garr[r] = G[k][i] for a record r of b's segment admitted into slot (k, i), exact 0 for a refused one.  garr [A]
 *       is indexed like a_cap; records outside the call's segments are not written.
 * step = -1 (the advance that built the first period's problems) reads no applied, status, x, max_pilot or gdir and
 * writes no gx.  plan->a_seg == NULL: no arrival in this step.  The peak series and the demand-charge floor (rules 7, 8)
 * get no adjoint.  tests/advance_vjp_spec.py states the rules in plain loops and the library returns its bits; no atomics.
 * Refused with ACNQP_ERR_INVALID and acnqp_last_error set, before any device work and with the outputs untouched: a null
 * handle, cur or plan; a site with a load-flattening or demand-charge row; n_evse or n_rows other than the handle's;
 * k_sessions above 4; x, applied, gdir, gx or max_pilot NULL at step >= 0; gprice without a clock cost; gprice and gq_next
 * without horizon_next; series_len < step + 1 + t_max; an output that overlaps an input or another output.  The clock
 * cost's series is not read.  _device: device pointers, enqueued on `hip_stream`, no synchronisation.  _host: host
 * pointers, synchronous, chunked like the other host entries; same bits.                                              */
int acnqp_advance_vjp_device(acnqp_handle* h, const acnqp_problems* cur, const double* applied, const int32_t* status,
                             const double* x, const acnqp_advance_plan* plan, const acnqp_clock_cost* cost,
                             const double* max_pilot, const double* gdir, const double* gq_next,
                             const double* gcap_vjp_next, const double* gcap_carry_next, const int32_t* horizon_next,
                             const int32_t* flags_next, double* gx, double* gcap_carry, double* garr, double* gprice,
                             void* hip_stream);
int acnqp_advance_vjp_host(acnqp_handle* h, const acnqp_problems* cur, const double* applied, const int32_t* status,
                           const double* x, const acnqp_advance_plan* plan, const acnqp_clock_cost* cost,
                           const double* max_pilot, const double* gdir, const double* gq_next,
                           const double* gcap_vjp_next, const double* gcap_carry_next, const int32_t* horizon_next,
                           const int32_t* flags_next, double* gx, double* gcap_carry, double* garr, double* gprice);

/* ---- before the solve (additive to ABI v10: new symbols only) --------------------------------------------------------
 * The link between the slot state an advance writes and the two steps of the reference that read the SESSION LIST:
 * apply_minimum_charging_rate (ada.py:147-150), a greedy walk in arrival order, and diff_based_reallocation
 * (post.py:214-218), whose round robin breaks ties of the rounding loss by list order.  The slot state carries no order:
 * the caller states it, as key[b][i] = the list position of the session on EVSE i of problem b.  The entry runs on the
 * problems `cur` an advance just wrote, before they are solved.  K = 1 only (online MPC: one session per EVSE).
 * A slot is LIVE when s_len > 0 and PRESENT when it is live and s_off == 0.  For every problem b, in this order:
 *    1  order: the live slots in ascending (key[i], i).  Comparisons only; key is read only where the slot is live.
 *    2  minimum rates, when min_pilot is given (acn.apply_minimum_charging_rate with its default override): with
 *       w = 0 [N], the present slots are visited in the order of rule 1.  A visit sets want = min_pilot[i], w[i] = want and
 *       tests  s_cap[i] >= want  and, for every row j,  re_j^2 + im_j^2 <= (limits_j + 1e-7)^2  with
 *       re_j = sum_i cre[j][i] w[i] (im_j likewise): the sums over increasing i, every product and every sum rounded once
 *       (no fused multiply-add, no square root) -- the acceptance test of the pilots entry without its peak term.
 *       Accepted:  lb[i][0] = max(want, lb[i][0]), then ub[i][0] = (ub[i][0] < lb[i][0] ? lb[i][0] : ub[i][0]).
 *       Refused:   w[i] = 0 and lb[i][0] = ub[i][0] = 0.
 *       Only period 0 of lb and ub is touched, and only of present slots.
 *    3  the session view, when wanted: positions b*N + r, r = 0 .. N-1 -- first the live slots in the order of rule 1, then
 *       the EVSEs without a live slot in increasing i.  v_evse = the EVSE, v_arrived = present,
 *       v_cap = present ? min(s_cap[i], ub'[i][0]) : 0 with ub' as rule 2 left it (max_pilot is inside ub already).  These
 *       are s_evse, s_arrived and s_cap of acnqp_pilot_plan with the constant sess_seg[b] = b*N.
 *    4  flags[b] is written for every problem: bit 1 when a live slot has s_off > 0 (no state of online MPC; the slot is
 *       left untouched by rule 2 and is not present in rule 3), else 0.
 * tests/prepare_spec.py states the rules in plain loops and the library returns its bits.  No atomics; every view element
 * is written whatever the input; a problem gives the same bits alone and at any position of any batch.                 */
#define ACNQP_PREPARE_FUTURE 1   /* flags: a live slot with s_off > 0 */

typedef struct {
  int32_t n_evse;           /* N: must be the handle's                                                                */
  int32_t n_infra;          /* M: must be the handle's                                                                */
  const int32_t* key;       /* [B*N]  list position of the session on EVSE i (read where the slot is live)            */
  const double* cre;        /* [M*N]  the site in the SOC form of acnqp_pilot_plan; read only with min_pilot          */
  const double* cim;        /* [M*N]                                                                                  */
  const double* limits;     /* [M]                                                                                    */
  const double* min_pilot;  /* [N] or NULL: no rule 2                                                                 */
} acnqp_prepare_plan;

typedef struct {
  int32_t* v_evse;     /* [B*N]                                                                                       */
  uint8_t* v_arrived;  /* [B*N]                                                                                       */
  double* v_cap;       /* [B*N]   all three or none (none: the view is not wanted)                                    */
} acnqp_prepare_view;

/* acnqp_prepare_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns without
 * synchronising.  cur: batch, t_max, k_sessions and s_off, s_len, s_cap are read (its lb / ub are not: they are const);
 * lb, ub [B*N*Tm] are the writable bounds of the same problems; view may be NULL.  A null handle or argument, n_evse or
 * n_infra other than the handle's, k_sessions != 1, a shape out of range, a view with a missing array, min_pilot without
 * the site arrays, or an output (lb, ub, the view, flags) that overlaps an input or another output return
 * ACNQP_ERR_INVALID with acnqp_last_error set, before any device work.                                               */
int acnqp_prepare_device(acnqp_handle* h, const acnqp_problems* cur, const acnqp_prepare_plan* plan, double* lb, double* ub,
                         acnqp_prepare_view* view, int32_t* flags, void* hip_stream);

/* acnqp_prepare_host -- the same with host pointers, synchronous; a large batch is processed in chunks.  Same bits as
 * the device entry.                                                                                                  */
int acnqp_prepare_host(acnqp_handle* h, const acnqp_problems* cur, const acnqp_prepare_plan* plan, double* lb, double* ub,
                       acnqp_prepare_view* view, int32_t* flags);

/* ---- the plant (additive to ABI v10: new symbols only, no new struct) ---------------------------------------------------
 * What every EV DRAWS of the pilot it is offered.  The advance's rule 1 takes `applied` as delivered; a closed loop that
 * hands it the pilots themselves models an EV that draws exactly what it is offered.  This entry puts a battery per EV in
 * between: a current limit, the room left to full and, in the two-stage model, a tail in which the accepted rate falls in
 * proportion to that room (acnportal's Battery and Linear2StageBattery in their stepwise form, as recalled: its rate cap
 * (1 - soc) / (1 - transition_soc) * max_power once soc >= transition_soc is room / knee * amps in the units below).
 * Units are the slot state's: amperes and ampere-periods.  K = 1 only (online MPC: one session per EVSE).
 * The caller owns a read-only battery TABLE of n_batteries rows, computed once per EV:
 *    t_room[r]   room left at plug-in, A-periods        t_amps[r]   the battery's current limit, A
 *    t_knee[r]   room at which the tail begins, or 0 for a battery without one (ideal)
 *    t_slope[r]  t_amps[r] / t_knee[r] where t_knee > 0, else 0 -- divided by the caller, once: the entry never divides
 * A row with t_room = t_amps = +inf and t_knee = 0 is "no battery model": it draws what it is offered.
 * The state is bat[e] (the row of the battery on EVSE i of problem b, e = b*N + i; -1: none) and room[e].
 * For every (b, i), in this order:
 *    1  plug:    r = plug[e].  r < 0: nothing changes.  0 <= r < n_batteries: bat[e] = r, room[e] = t_room[r].
 *                r >= n_batteries: ignored, flag ACNQP_PLANT_BAD_PLUG.
 *    2  offer:   p = pilots[e] when the slot is present (s_len[e] > 0 and s_off[e] == 0), status is NULL or status[b] is
 *                SOLVED or SOLVED_INACCURATE, and pilots[e] > 0; else p = 0 (rule 1 of the advance: time passes,
 *                nothing is delivered).
 *    3  draw:    r = bat[e] as rule 1 left it.  r < 0: a = p.  r >= n_batteries: a = p, flag ACNQP_PLANT_BAD_BATTERY (the
 *                entry leaves such a bat[e] and its room[e] as they came).  Otherwise
 *                  lim = t_amps[r];  where t_knee[r] > 0 and room[e] <= t_knee[r]:  lim = min(lim, room[e] * t_slope[r])
 *                  a = max(min(p, lim, room[e]), 0);  room[e] = room[e] - a
 *                -- comparisons, ONE product and ONE subtraction, each rounded once (no fused multiply-add).
 *    4  output:  actual[e] = a; bat[e] and room[e] are written back.
 *    5  flags[b] is written for every problem, 0 when nothing was flagged.
 * tests/plant_spec.py states the rules in plain loops and the library returns its bits.  No atomics; every output element
 * is written whatever the input; a problem gives the same bits alone and at any position of any batch.  Inputs are
 * finite or +inf: the library is built without NaN semantics, a NaN pilot is not served.                               */
#define ACNQP_PLANT_BAD_PLUG 1      /* flags: plug[e] >= n_batteries (ignored)                                          */
#define ACNQP_PLANT_BAD_BATTERY 2   /* flags: bat[e] >= n_batteries (drawn as if there were no battery)                 */

/* acnqp_plant_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns without
 * synchronising.  cur: batch, k_sessions (must be 1), s_off and s_len are read.  pilots, plug, bat, room, actual: [B*N];
 * status: [B] or NULL; the four tables: [n_batteries]; flags: [B].  Refused with ACNQP_ERR_INVALID and acnqp_last_error
 * set, before any device work: a null handle or required pointer, k_sessions != 1, a negative batch or n_batteries,
 * n_batteries > 0 with a null table, an output (bat, room, actual, flags) that overlaps an input or another output.
 * batch == 0 returns ACNQP_OK.                                                                                       */
int acnqp_plant_device(acnqp_handle* h, const acnqp_problems* cur, const double* pilots, const int32_t* status,
                       int32_t n_batteries, const double* t_room, const double* t_amps, const double* t_knee,
                       const double* t_slope, const int32_t* plug, int32_t* bat, double* room, double* actual,
                       int32_t* flags, void* hip_stream);

/* acnqp_plant_host -- the same with host pointers, synchronous; a large batch is processed in chunks (the tables are
 * uploaded once per call).  Same bits as the device entry, at any chunking.                                         */
int acnqp_plant_host(acnqp_handle* h, const acnqp_problems* cur, const double* pilots, const int32_t* status,
                     int32_t n_batteries, const double* t_room, const double* t_amps, const double* t_knee,
                     const double* t_slope, const int32_t* plug, int32_t* bat, double* room, double* actual,
                     int32_t* flags);

/* ---- the ramp-down estimator (additive to ABI v10: new symbols only, no new struct) ---------------------------------------
 * The reference's estimate_max_rate (ada.py:143-146): an estimator of what each EV accepts caps the session's max_rates
 * before the solve, then reconcile_max_and_min(choose_min = True).  The estimator is acnportal's SimpleRampdown, as
 * recalled: an EV that drew clearly less than it was offered has its bound set to just above what it drew; an EV that
 * draws all its bound allows has the bound raised by up_increment.  With the plant above, this closes the loop in which an
 * EV in the tail of its battery stops holding infrastructure capacity it will not use.
 * Units are the slot state's: amperes.  K = 1 only (online MPC: one session per EVSE).
 * Parameters: up_threshold, down_threshold (either may be +-inf: with down_threshold = +inf and up_threshold = -inf the
 * estimate never moves) and up_increment (finite, >= 0), in amperes.
 * The state is est[e], the bound of the session on EVSE i of problem b, e = b*N + i; +inf where there is none.  It starts
 * at +inf.  For every (b, i), in this order:
 *    1  slot:    present = s_len[e] > 0 and s_off[e] == 0 and s_len[e] <= t_max.  Every other slot counts as absent: none
 *                (s_len <= 0), one still to come (s_off > 0), and one whose window does not fit: s_len[e] > t_max, whatever
 *                its s_off, flag ACNQP_ESTIMATE_BAD_SLOT.
 *    2  absent:  est'[e] = +inf and ub_out[e][:] = ub[e][:], a copy.  fresh[e] != 0 here: flag ACNQP_ESTIMATE_BAD_FRESH.
 *    3  first sight, present and fresh[e] != 0:  u = ub[e][0] -- the session's own max_rates[0] after enforce_pilot_limit.
 *                No history is read.
 *    4  update, present and not fresh:  u = est[e].  pilots == NULL (no history: the first step of a run): u is kept.
 *                Otherwise, with served = status is NULL or status[b] is SOLVED or SOLVED_INACCURATE:
 *                  pp = pilots[e] when served and pilots[e] > 0, else 0           (what was offered: the plant's rule 2)
 *                  pr = pp when actual is NULL (what is offered is drawn), else actual[e] when served, else 0
 *                  if      pp - pr > down_threshold:  u = pr + up_increment       (ramp down to just above what was drawn)
 *                  else if u  - pr < up_threshold:    u = u + up_increment        (the EV draws what it may: probe upwards)
 *                  else                               u is kept
 *                -- at most two subtractions, two comparisons and one addition, each rounded once.
 *    5  output:  est'[e] = u.  For t < s_len[e]:  v = (u < ub[e][t] ? u : ub[e][t]), then
 *                ub_out[e][t] = (v < lb[e][t] ? lb[e][t] : v) -- reconcile_max_and_min with choose_min = True.
 *                For t >= s_len[e]:  ub_out[e][t] = ub[e][t].
 *    6  flags[b] is written for every problem, 0 when nothing was flagged.
 * ub_out is an array of its own: the state keeps the session's own bounds (the advance shifts THEM into the next period,
 * and the estimate may rise again), only the solve reads the capped copy.  lb is read and never written.
 * tests/estimate_spec.py states the rules in plain loops and the library returns its bits.  No atomics; every output
 * element is written whatever the input; a problem gives the same bits alone and at any position of any batch.  est may
 * hold +inf; every other input is finite: the library is built without NaN semantics.                                 */
#define ACNQP_ESTIMATE_BAD_FRESH 1   /* flags: fresh[e] != 0 on an absent slot                                           */
#define ACNQP_ESTIMATE_BAD_SLOT 2    /* flags: s_len[e] > t_max (counted as absent)                                      */

/* acnqp_estimate_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns
 * without synchronising.  cur: batch, k_sessions (must be 1), t_max, s_off, s_len, lb and ub are read.  fresh, est: [B*N];
 * pilots, actual: [B*N] or NULL; status: [B] or NULL; ub_out: [B*N*t_max]; flags: [B].  Refused with ACNQP_ERR_INVALID and
 * acnqp_last_error set, before any device work: a null handle or required pointer, k_sessions != 1, a negative batch,
 * t_max outside [1, 4096], actual given without pilots, an output (est, ub_out, flags) that overlaps an input or another
 * output.  batch == 0 returns ACNQP_OK.                                                                              */
int acnqp_estimate_device(acnqp_handle* h, const acnqp_problems* cur, const int32_t* fresh, const double* pilots,
                          const double* actual, const int32_t* status, double up_threshold, double down_threshold,
                          double up_increment, double* est, double* ub_out, int32_t* flags, void* hip_stream);

/* acnqp_estimate_host -- the same with host pointers, synchronous; a large batch is processed in chunks.  Same bits as
 * the device entry, at any chunking.                                                                                 */
int acnqp_estimate_host(acnqp_handle* h, const acnqp_problems* cur, const int32_t* fresh, const double* pilots,
                        const double* actual, const int32_t* status, double up_threshold, double down_threshold,
                        double up_increment, double* est, double* ub_out, int32_t* flags);

/* ---- select and hold (additive to ABI v10: new symbols only, no new struct) ------------------------------------------------
 * The loop around the reference's schedule() does not solve every period: the plant calls the algorithm when an EV plugs
 * in, when one unplugs, or when max_recompute periods have passed since the last solve, and plays the rest of the schedule
 * it holds in between.  Which scenario of a batch resolves at which step follows from arrivals, departures and
 * max_recompute, all known before the run, so the caller knows the size of every step's solve without reading an answer.
 * These two entries are the device side of that loop: SELECT takes the resolving problems out of the resident state into a
 * dense batch of m problems, acnqp_solve_batch_device solves that batch, and HOLD puts the answers back into the full
 * batch beside the held schedules of everyone else.
 *
 * select -- cur: the state, B = cur->batch problems; idx[0:m]; out, s_eq, flags: the dense batch, m problems.  For j in
 * [0, m) with b = idx[j]:
 *    S1  0 <= b < B:  every array of acnqp_problems is copied from row b to row j, bit for bit: horizon, lb, ub, q, pdiag,
 *        s_off, s_len, s_cap, s_eq; peak, lf, dc, dfloor exactly where the site has the row; warm_x and warm_y when wanted
 *        (out->warm_x / out->warm_y not NULL: then cur->warm_x / cur->warm_y are their sources); flags[j] = 0.
 *    S2  otherwise:  flags[j] = ACNQP_SELECT_BAD_INDEX and problem j is the empty problem: horizon 1, zeros, peak +inf, no
 *        live slot, s_eq and dfloor 0, warm arrays 0.  Nothing of cur is read for it.
 * hold -- cur: the state (batch, t_max, lb and ub are read); pos[0:B]: the row of scenario b in the dense batch, or -1;
 * dense: the dense results x, status, iters and, when wanted, y (m rows, read only); held_x and, when wanted, held_y: the
 * schedule every scenario holds -- the warm_x' / warm_y' the advance wrote under its rule 9; prev_status[0:B]; out: x,
 * status, iters and, when wanted (out->y not NULL on a site with rows), y of all B; solved, flags: [B].  For every b with
 * j = pos[b]:
 *    H1  0 <= j < m:  x[b] = dense->x[j], y[b] = dense->y[j], status[b] = dense->status[j], iters[b] = dense->iters[j],
 *        solved[b] = 1.
 *    H2  otherwise, for every element v = held_x[b][i][t]:  if v > ub then v = ub, then if v < lb then v = lb -- comparisons
 *        only, in this order -- and x[b][i][t] = v.  y[b] = held_y[b], status[b] = prev_status[b], iters[b] = 0,
 *        solved[b] = 0.  The clip gives a held schedule the invariants of a solver output: lb <= x <= ub exactly and exact
 *        zeros outside live windows (a session the advance retired early has ub = 0 on its window, advance rule 3).
 *    H3  a j outside [-1, m) is held as in H2 and sets flags[b] = ACNQP_HOLD_BAD_ROW; otherwise flags[b] = 0.
 * A held schedule is NOT the schedule a fresh solve would give: it does not see that a battery drew less than it was
 * offered, nor that the tariff has moved.  It is what the reference's user applies between two calls of schedule().
 * A scenario whose last solve was not accepted keeps that status while it is held: the advance delivers nothing for it
 * (advance rule 1) until its next scheduled solve.  The mask of who resolves never depends on the answers -- that is what
 * keeps a loop built on these entries free of host synchronisation.
 * tests/hold_spec.py states both rule lists in plain loops and the library returns its bits: every element is a copy, a
 * constant or the outcome of two comparisons.  No atomics; every output element is written whatever the input; a problem's
 * output does not depend on j, b or m.  Inputs are finite or +inf: the library is built without NaN semantics.          */
#define ACNQP_SELECT_BAD_INDEX 1   /* flags of select: idx[j] outside [0, batch) (problem j is the empty problem)       */
#define ACNQP_HOLD_BAD_ROW 1       /* flags of hold: pos[b] outside [-1, m) (scenario b is held)                        */

/* acnqp_select_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns without
 * synchronising.  cur: all of it is read (warm_x / warm_y only when wanted).  out: the arrays of the dense batch, [m*...]
 * in the layout of acnqp_problems; s_eq: [m]; flags: [m].  Refused with ACNQP_ERR_INVALID and acnqp_last_error set, before
 * any device work: a null handle or argument; n_evse or n_rows other than the handle's; a negative batch, t_max or
 * k_sessions outside [1, 4096], m < 0 or m > batch; a null required array; a site row without its array (in cur or out);
 * on a site with rows, out->warm_x without out->warm_y or the reverse; a warm output without its source; an output that
 * overlaps an input or another output.  m == 0 is a valid call and launches nothing.                                   */
int acnqp_select_device(acnqp_handle* h, const acnqp_problems* cur, int32_t n_evse, int32_t n_rows, int32_t m,
                        const int32_t* idx, acnqp_next* out, uint8_t* s_eq, int32_t* flags, void* hip_stream);

/* acnqp_select_host -- the same with host pointers, synchronous; the state is uploaded once, a large dense batch is
 * processed in chunks.  Same bits as the device entry, at any chunking.  Here idx can be read: one that is not strictly
 * increasing is refused too.                                                                                         */
int acnqp_select_host(acnqp_handle* h, const acnqp_problems* cur, int32_t n_evse, int32_t n_rows, int32_t m,
                      const int32_t* idx, acnqp_next* out, uint8_t* s_eq, int32_t* flags);

/* acnqp_hold_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns without
 * synchronising.  Refused with ACNQP_ERR_INVALID and acnqp_last_error set, before any device work: a null handle or
 * argument; n_evse or n_rows other than the handle's; a negative batch, t_max or k_sessions outside [1, 4096], m < 0 or
 * m > batch; a null required array (the dense results are required only when m > 0); y wanted without held_y or, when
 * m > 0, dense->y; an output (out->x, status, iters, y, solved, flags) that overlaps an input or another output.
 * batch == 0 returns ACNQP_OK; m == 0 is a valid call and holds everyone.                                              */
int acnqp_hold_device(acnqp_handle* h, const acnqp_problems* cur, int32_t n_evse, int32_t n_rows, int32_t m,
                      const int32_t* pos, const acnqp_results* dense, const double* held_x, const double* held_y,
                      const int32_t* prev_status, acnqp_results* out, uint8_t* solved, int32_t* flags, void* hip_stream);

/* acnqp_hold_host -- the same with host pointers, synchronous; the dense results are uploaded once, a large batch is
 * processed in chunks.  Same bits as the device entry, at any chunking.  Here pos can be read: one that is not the inverse
 * of a strictly increasing idx[0:m] -- its entries inside [0, m) count 0, 1, ... m - 1 as b rises -- is refused too.     */
int acnqp_hold_host(acnqp_handle* h, const acnqp_problems* cur, int32_t n_evse, int32_t n_rows, int32_t m,
                    const int32_t* pos, const acnqp_results* dense, const double* held_x, const double* held_y,
                    const int32_t* prev_status, acnqp_results* out, uint8_t* solved, int32_t* flags);

/* ---- gradients through the solve (additive to ABI v10: new symbols only) ---------------------------------------------
 * For an answer (x, y) of the library and gx = dL/dx of a scalar L of the schedule: the gradients of L with respect to the
 * problem's data, by one adjoint solve with the KKT matrix of the optimal working set, in the minimisation form and the
 * units of this header.  With pd_eff as in the dual report, the working set is taken at (x, y) as the Newton polish takes
 * its first guess: a variable within 1e-7 of a bound is fixed; an energy row is tight when s_eq holds or its sum reaches
 * cap - 1e-7 max(1, |cap|); a site row or peak period is tight when its multiplier in y (a SOC pair: its length) exceeds
 * 1e-9 max(1, |q|_inf).  A tight SOC pair enters by its outward normal at G x and, with a multiplier above
 * 1e-7 max(1, |q|_inf), by its curvature.  With H = pd_eff I + the curvature and C the tight rows on the free variables,
 *
 *     H a + C'm = gx_free,   C a = 0        (dual regularisation as in the polish: dependent rows get the least-norm m)
 *
 *   gq    [B*N*Tm]       dL/dq = -a on free variables; exact 0 on fixed ones, at t >= horizon[b] and outside every window
 *   gcap  [B*K*N]        layout of s_cap: dL/dcap = m of the session's row; 0 for a slack row and an empty slot
 *   grow  [B*nrow*Tm]    nrow = n_infra + has_peak: dL/d(limit of row r at period t) = m of that row; 0 where it is not
 *                        tight.  limits[r] is shared by all periods: its gradient is the sum over t.  Row n_infra is the
 *                        peak row: the gradient of peak[t] is its own entry.  May be NULL when nrow is 0
 *   glb, gub  [B*N*Tm]   either may be NULL: for a variable fixed at that bound (lb wins where both hold) gx minus the
 *                        variable's column of (H, C) applied to (a, m); 0 elsewhere
 *   info  [B*4] int32    [0] verdict: 0 done, 1 status neither SOLVED nor SOLVED_INACCURATE, 2 the working set outgrows
 *                        the kernel's tables (the polish's limits), 3 a pivot of the factorisation is not positive;
 *                        [1] rows of the Schur system; [2] weak members: fixed variables with lb < ub and tight
 *                        inequality energy rows whose own multiplier at (x, y), from stationarity, is below
 *                        1e-9 max(1, |q|_inf) in magnitude -- there the solution map has a kink and the gradient is that
 *                        of the working set as taken; [3] free variables
 *   res   [B*2]          [0] |H a + C'm - gx|_inf on the free variables / max(1, |gx|_inf), of the solve as performed;
 *                        [1] |pd_eff x + q + G'y + mu|_inf on the free variables / max(1, |q|_inf), mu the least-squares
 *                        multipliers of the tight energy rows: how far from a KKT point the gradient was taken
 * A verdict other than 0 writes exact zeros to that problem's gradients, counts and residuals.  No floating-point
 * atomics, fixed summation order: the same problem gives the same bits in any batch, at any position.
 *
 * acnqp_vjp_device -- every pointer is a device pointer on the handle's GPU; enqueued on `hip_stream`, returns without
 * synchronising.  p: the problems (warm_x / warm_y ignored); o: read for reg_rel only; x, y (may be NULL for a site
 * without rows) and status (NULL: every problem counts as solved) as a solve wrote them.  Served: n_evse <= 64,
 * t_max <= 32 (to 288 behind acnqp_set_long_vjp, below), k_sessions <= 4, no flat and no max row.  Refused with ACNQP_ERR_INVALID and acnqp_last_error set,
 * outputs untouched: a null handle or argument, a shape not served, a null required array, an output that overlaps an
 * input or another output.  batch == 0 returns ACNQP_OK.                                                               */
int acnqp_vjp_device(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, const double* x, const double* y,
                     const int32_t* status, const double* gx, double* gq, double* gcap, double* grow, double* glb,
                     double* gub, int32_t* info, double* res, void* hip_stream);

/* acnqp_vjp_host -- the same with host pointers, synchronous; a large batch is processed in chunks.  Same bits as the
 * device entry.                                                                                                       */
int acnqp_vjp_host(acnqp_handle* h, const acnqp_problems* p, const acnqp_options* o, const double* x, const double* y,
                   const int32_t* status, const double* gx, double* gq, double* gcap, double* grow, double* glb,
                   double* gub, int32_t* info, double* res);

/* Additive to ABI v10 (a new symbol; no structure changes): gradients through the solve at horizons 33 ... 288.  A property
 * of the handle, OFF after acnqp_create: with it off acnqp_vjp_device / acnqp_vjp_host are what they were, and t_max > 32 is
 * refused with "horizons 1 ... 32 are served".  on != 0: the two entries also serve 33 <= t_max <= 288 on a site with
 * n_evse <= 64, k_sessions <= 4, at least one row (n_infra + has_peak >= 1), at most 48 rows of acnqp_site.G and no flat or
 * max row, by a second kernel that keeps its state in a slab of global memory per workgroup (min(batch, compute units)
 * workgroups, fewer where the slabs would pass 512 MiB; the slabs are the handle's, per stream, and the device entry
 * synchronises the stream only when they must grow).  Outputs, masks, info and res as above; its tables hold the worst case
 * of the shape, so verdict 2 does not occur there; same bits in any batch, at any position, from either entry.  For
 * t_max <= 32 the switch changes nothing: the same kernel, the same bits.  New refusals with it on (ACNQP_ERR_INVALID,
 * outputs untouched, the reason in acnqp_last_error): t_max > 288 ("horizons 1 ... 288 are served"); and at t_max > 32 a
 * site without rows, or with more than 48 rows of G.  Returns ACNQP_OK, ACNQP_ERR_INVALID for a null handle.            */
int acnqp_set_long_vjp(acnqp_handle* h, int32_t on);

#ifdef __cplusplus
}
#endif
#endif /* ACN_QP_H */
