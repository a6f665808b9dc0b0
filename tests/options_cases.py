"""Solver options other than the defaults: the pools, the option sets and the CPU reference of
tests/test_options_cases.py (the reference alone: every option set is told apart from its neighbour by oracle/admm_port,
the classification probes are robust, oracle/admm_ref grounds the twin) and tests/test_options_gpu.py (every kernel route
follows the twin under every option set).  A plain module, like verdict_cases.py and wave_cases.py.

``acnqp_options`` has 19 fields and each of the five solver kernels reads them for itself.  The twin
(oracle/admm_port.c) takes every one of them; with ``accel_mem = 0`` the kernels follow it to the summation order.

Layers (tests/test_options_gpu.py):
  A  truncated trajectories -- ``accel_mem = 0, polish_iters = 0, retry_passes = 0`` and a limit of three check periods
     (plus 60 at period 7 and 30 at period 50): iterate, multipliers and residuals against the twin's at TRAJ_TOL;
  B  full solves without Anderson columns and polish: status, certificate and iteration count;
  C  as shipped (Anderson columns, polish) at check periods 7 and 1.
"""
import functools

import numpy as np

from tests import helpers as H
from tests import verdict_cases as V

# ---- pools ----------------------------------------------------------------------------------------------------------
# name -> kernel families to launch (None: every family the pool reaches).  Between them all eleven.
POOLS = {
    "n8_soc": None,                                   # one row tile: wave1/2/5, tiled_ct1/2, long_ws, general (289 periods)
    "pods18_lin": {"wave3", "wave4", "long_lds"},     # two row tiles
    "wide80_soc": {"stream"},                         # 80 EVSEs
    "n2_t40_lin": {"wave5", "long_ws"},               # horizon 40
    "ct54_lp": {"wave1", "wave2", "tiled_ct1", "long_ws"},   # caltech54, pdiag = 2e-12: the Tikhonov floor acts
    "stalled": {"wave3", "wave4", "long_lds", "tiled_ct1"},   # N = 36, two row tiles: stall rule and retry passes act
}
_FILLER = {"n8_soc": ("n8", "SOC", 24), "pods18_lin": ("pods18", "LINEAR", 24), "wide80_soc": ("wide80", "SOC", 24),
           "n2_t40_lin": ("n2_t40", "LINEAR", 16)}


@functools.lru_cache(maxsize=None)
def pool(name):
    from adacharge_amd.builder import ProblemBatch
    from tests import wave_cases

    if name in _FILLER:
        site, cone, n = _FILLER[name]
        return ProblemBatch.concatenate(V.solved_filler(site, cone, np.random.default_rng(77), n))
    if name == "ct54_lp":
        return wave_cases.build("soc")[0].subset(slice(0, 24))
    if name == "stalled":
        return wave_cases.build("stalled")[0]
    raise KeyError(name)


# ---- option sets ----------------------------------------------------------------------------------------------------
VARIANTS = {
    "defaults": {},
    "alpha1.0": dict(alpha=1.0),
    "alpha1.8": dict(alpha=1.8),
    "sigma1e-3": dict(sigma=1e-3),
    "rho0.2_fixed": dict(rho=0.2, adapt_every=0),
    "rho0.5": dict(rho=0.5),
    "adapt40": dict(adapt_every=40),
    "adapt30": dict(adapt_every=30),          # inside a check only: adapts at 60, 120, ...
    "ce7_ae7": dict(check_every=7, adapt_every=7),
    "ce7_ae20": dict(check_every=7, adapt_every=20),   # adapts at 140, 280, ...
    "adapt_tol1.5": dict(adapt_tol=1.5),
    "eps1e-5": dict(eps_abs=1e-5, eps_rel=1e-5),
    "eps1e-10": dict(eps_abs=1e-10, eps_rel=1e-10),
    "ce1_ae1": dict(check_every=1, adapt_every=1),
    "ce50": dict(check_every=50),             # with the limit 30 below it: one check, at the limit
    # Layer A: at the defaults no problem of the pools leaves the band (ratio within 1/3 ... 3) in its first 60 iterations,
    # so the schedule of the adaptation shows only from a start off balance: rho = 0.5 with the band at 1.5, and for a
    # check at every iteration, where only iterations 1 and 2 can adapt, rho = 0.005
    "off": dict(rho=0.5, adapt_tol=1.5),
    "off_adapt40": dict(rho=0.5, adapt_tol=1.5, adapt_every=40),
    "off_adapt30": dict(rho=0.5, adapt_tol=1.5, adapt_every=30),
    "off_ce7_ae7": dict(rho=0.5, adapt_tol=1.5, check_every=7, adapt_every=7),
    "off_ce7_ae20": dict(rho=0.5, adapt_tol=1.5, check_every=7, adapt_every=20),
    "off_ce50": dict(rho=0.5, adapt_tol=1.5, check_every=50),
    "low": dict(rho=0.005, adapt_tol=1.5),
    "low_ce1_ae1": dict(rho=0.005, adapt_tol=1.5, check_every=1, adapt_every=1),
    # ct54_lp only
    "reg0": dict(reg_rel=0.0),
    "reg0.001": dict(reg_rel=0.001),
    "reg0.5": dict(reg_rel=0.5),
    "reg2": dict(reg_rel=2.0),
    # the stalled pool: stall rule, retry passes, the floor of SOLVED_INACCURATE
    "stall200": dict(stall_iters=200),
    "stall200_retry1": dict(stall_iters=200, retry_passes=1, retry_rho=2.0, retry_max_iter=500),
    # (floor 0: 100 eps decides between 2 and 5.  At eps = 1e-8 two of the ten problems end on that line -- another status
    #  with eps halved or doubled --, at 3e-9 one does)
    "noretry_floor0": dict(retry_passes=0, inaccurate_floor=0.0, eps_abs=3e-9, eps_rel=3e-9),
    "noretry_floor1e-3_stall200": dict(retry_passes=0, inaccurate_floor=1e-3, stall_iters=200),
    # n8_soc under a short limit: the floor decides between MAX_ITER and SOLVED_INACCURATE
    "short100_floor0": dict(max_iter=100, retry_passes=0, inaccurate_floor=0.0),
    "short100_floor1e-2": dict(max_iter=100, retry_passes=0, inaccurate_floor=1e-2),
    "short100_floor_default": dict(max_iter=100, retry_passes=0),
    # n8_soc under a short limit: what is unsolved after 240 iterations is retried
    "retry2_140": dict(max_iter=240, stall_iters=200, retry_passes=2, retry_max_iter=140),   # unsolved: 240 + 140
    "retry2_400": dict(max_iter=240, stall_iters=200, retry_passes=2, retry_max_iter=400),   # 240 + 240 + 240
    "retry1_400": dict(max_iter=240, stall_iters=200, retry_passes=1, retry_max_iter=400),   # 240 + 240
    "retry_stall0": dict(max_iter=240, stall_iters=0, retry_passes=2, retry_max_iter=400),   # none retries (window 3000)
    # a fixed penalty switches the retry passes off (include/acn_qp.h: adapt_every = 0)
    "fixed_no_retry": dict(adapt_every=0, max_iter=240, stall_iters=200, retry_passes=2, retry_max_iter=400,
                           inaccurate_floor=1e-3),   # (all SOLVED_INACCURATE after 240, far from the floor)
    # ... retry_rho: a retry pass is kept only where it ends better than the pass before, so with the sets above status,
    # count and iterate are the same for every retry_rho.  Here pass 0 is held at a poor fixed penalty (rho = 1e-4, a band
    # no ratio leaves; adapt_every stays > 0, which a retry needs) and ends MAX_ITER; the retry ends SOLVED_INACCURATE
    # under the floor 0.03 and its iterate after 240 iterations at the fixed retry_rho is the answer.
    "retry_rho0.5": dict(rho=1e-4, adapt_tol=1e9, max_iter=240, stall_iters=200, retry_passes=1, retry_max_iter=400,
                         inaccurate_floor=0.03, retry_rho=0.5),
    "retry_rho0.2": dict(rho=1e-4, adapt_tol=1e9, max_iter=240, stall_iters=200, retry_passes=1, retry_max_iter=400,
                         inaccurate_floor=0.03, retry_rho=0.2),
}
# the neighbour a set is told apart from, where it is not the defaults
NEIGHBOUR = {"off_adapt40": "off", "off_adapt30": "off", "off_ce7_ae7": "off", "off_ce7_ae20": "off", "off_ce50": "off",
             "low_ce1_ae1": "low", "retry_rho0.5": "retry_rho0.2", "retry_rho0.2": "retry_rho0.5", "retry2_140": "retry_stall0",
             "retry2_400": "retry2_140", "retry1_400": "retry2_400", "retry_stall0": "retry2_140", "fixed_no_retry": "retry2_400",
             "short100_floor0": "short100_floor1e-2", "short100_floor1e-2": "short100_floor0",
             "short100_floor_default": "short100_floor1e-2"}

COMMON_A = ("alpha1.0", "alpha1.8", "sigma1e-3", "rho0.2_fixed", "rho0.5", "adapt_tol1.5", "off_adapt40", "off_adapt30",
            "off_ce7_ae7", "off_ce7_ae20", "off_ce50", "low_ce1_ae1")
LAYER_A = {"n8_soc": COMMON_A, "pods18_lin": COMMON_A, "wide80_soc": COMMON_A, "n2_t40_lin": COMMON_A,
           "ct54_lp": ("reg0", "reg0.001", "reg0.5")}
LAYER_A_BASE = dict(accel_mem=0, polish_iters=0, retry_passes=0)


def check_period(variant):
    return int(VARIANTS[variant].get("check_every", 20))


def layer_a_limits(variant):
    """the iteration limits of layer A: three check periods; 60 too at period 7; 30 too at period 50"""
    ce = check_period(variant)
    return (3 * ce,) + ((60,) if ce == 7 else ()) + ((30,) if ce == 50 else ())


def layer_a_runs(pool_name):
    """[(variant, limit)] of a pool, the defaults first (the summation-order floor behind TRAJ_TOL)"""
    return [("defaults", 60)] + [(v, m) for v in LAYER_A[pool_name] for m in layer_a_limits(v)]


# Layer B: full solves.  A pairing (variant, pool) is listed only where the twin tells at least half of the pool apart from
# the neighbour by what the GPU test asserts there (status; iteration count beyond twice the bound; for the reg_rel sets the
# schedule beyond 10 RATE_TOL) -- tests/test_options_cases.py holds the list to that and prints every share.  Left out
# after measuring (share in brackets): see LAYER_B_LEFT_OUT.
LAYER_B_BASE = dict(accel_mem=0, polish_iters=0)
COMMON_B = ("alpha1.0", "alpha1.8", "sigma1e-3", "rho0.2_fixed", "rho0.5", "adapt40", "adapt30", "ce7_ae7", "ce7_ae20",
            "adapt_tol1.5", "eps1e-5", "eps1e-10")
LAYER_B_LEFT_OUT = {
    ("alpha1.8", "n8_soc"): 0.46, ("alpha1.8", "pods18_lin"): 0.08, ("sigma1e-3", "pods18_lin"): 0.12,
    ("adapt40", "pods18_lin"): 0.08, ("adapt30", "pods18_lin"): 0.08, ("ce7_ae7", "pods18_lin"): 0.33,
    ("ce7_ae20", "pods18_lin"): 0.29, ("sigma1e-3", "n2_t40_lin"): 0.44, ("adapt40", "n2_t40_lin"): 0.44,
    ("adapt_tol1.5", "n2_t40_lin"): 0.25,
    ("reg0.5", "ct54_lp"): 0.42,   # (told apart in layer A; reg_rel = 2 stands in for it here)
}
LAYER_B = {p: tuple(v for v in COMMON_B if (v, p) not in LAYER_B_LEFT_OUT) for p in ("n8_soc", "pods18_lin", "wide80_soc", "n2_t40_lin")}
LAYER_B["ct54_lp"] = ("reg0", "reg0.001", "reg2")
STALL_SETS = ("stall200", "stall200_retry1", "noretry_floor0", "noretry_floor1e-3_stall200")
FLOOR_SETS = ("short100_floor0", "short100_floor1e-2", "short100_floor_default")
RETRY_SETS = ("retry2_140", "retry2_400", "retry1_400", "retry_stall0", "fixed_no_retry", "retry_rho0.5", "retry_rho0.2")
LAYER_C = ("ce7_ae7", "ce1_ae1")

# ---- tolerances -----------------------------------------------------------------------------------------------------
RATE_TOL = 1e-4 * 32.0   # north star: 1e-4 relative on rates, 32 A pilots
# Layer A, measured on an MI355X.  |x - x_twin|_inf in A: ten times the worst value of the defaults runs over all routes
# (TRAJ_MEASURED: per route, at the defaults and over all sets); tests/test_options_cases.py caps it at a tenth of the
# smallest told-apart distance (9e-3 A).  Ten routes follow the twin to 4e-11 A; the large-site kernel does so on all but
# one or two problems of a run, which end 5e-9 ... 4e-8 A away (its session projection stops at a tolerance of its own:
# another point inside that tolerance, carried through 60 iterations).
# y relative to max(1, |y_twin|_inf) of the problem: ten times the worst of the defaults runs (1.71e-8, large-site kernel;
# elsewhere <= 1.6e-13).  pri_res and dua_res of a problem the twin leaves unsolved, relative to their own value: the worst
# of the defaults runs is 3.57e-8, over all sets 1.07e-6 (both the large-site kernel: alpha = 1, the problem whose iterate
# is 3.9e-8 A away; elsewhere <= 3.7e-11) -- ten times the latter, since a residual moves with the iterate and the iterate is
# already held to ten times its floor.  (A problem SOLVED within the limit has residuals of 1e-11 ... 1e-14, roundoff on
# either side: its status says that they are below eps.)
TRAJ_TOL = 5.3e-8
TRAJ_Y_REL = 1.8e-7
TRAJ_RES_REL = 1.1e-5
TRAJ_MEASURED = {   # route: (|x - x_twin| at the defaults, over all sets) in A
    "wave1": (2.79e-11, 3.30e-11), "wave2": (2.79e-11, 3.30e-11), "wave3": (1.17e-13, 8.05e-13), "wave4": (1.17e-13, 8.05e-13),
    "wave5": (1.58e-12, 8.09e-12), "tiled_ct1": (1.52e-11, 3.55e-11), "tiled_ct2": (3.00e-12, 9.35e-12),
    "long_lds": (1.46e-13, 6.64e-13), "long_ws": (3.66e-11, 3.66e-11), "general": (4.50e-12, 1.41e-11),
    "stream": (5.23e-09, 3.88e-08),
}
# Layer B, |iters - iters_twin| in check periods of the variant.  Measured on an MI355X: 0 on every route of every pool and
# set outside ITER_FRAGILE (below), 20 on the large-site kernel.
ITER_BOUND_PERIODS = 1

# ---- problems whose iteration count hangs on an adaptation decision ---------------------------------------------------
# The penalty adapts when sqrt(pri / dua) leaves a band; a problem whose ratio meets the band's edge at some check adapts or
# not by the last bits, and from there on runs another trajectory to the same optimum -- hundreds of iterations apart.
# The twin shows it on itself: with the cost vector moved by PERTURB = 1e-13 relative (a few hundred ulps; the kernels'
# sums differ from the twin's by their order, layer A measures 1e-11 A after 60 iterations) its count of such a problem
# moves (n8_soc alpha = 1: by 260 and 1200; wide80_soc at period 7: 2198; ct54_lp reg_rel = 0.001: 9580), and the count of
# every other problem stays where it is, to the iteration.  The MI355X agrees: at the defaults every route of n8_soc,
# pods18_lin, n2_t40_lin and ct54_lp gives the twin's count exactly, and the routes differ from it by hundreds of
# iterations on these problems alone.  ITER_FRAGILE lists them: {(pool, variant): indices whose count moves at all under
# any of PERTURB_SEEDS}; tests/test_options_cases.py holds the table to what the twin does and counts them as NOT told
# apart.  Everywhere else a kernel owes the twin's count within one check period.
PERTURB = 1e-13
PERTURB_SEEDS = tuple(range(4))
ITER_FRAGILE = {
    ("n8_soc", "alpha1.0"): (18,),
    ("wide80_soc", "defaults"): (18,),
    ("wide80_soc", "alpha1.0"): (9, 13, 18),
    ("wide80_soc", "sigma1e-3"): (18,),
    ("wide80_soc", "rho0.5"): (18,),
    ("wide80_soc", "adapt40"): (18,),
    ("wide80_soc", "adapt30"): (18,),
    ("wide80_soc", "ce7_ae7"): (14, 18, 22),
    ("wide80_soc", "eps1e-5"): (18,),
    ("wide80_soc", "eps1e-10"): (18,),
    ("ct54_lp", "reg0"): (9,),
    ("ct54_lp", "reg0.001"): (9,),
}


def iter_fragile(pool_name, variant, **extra):
    base = twin(pool_name, variant, **extra)["iters"]
    moved = np.zeros(len(base), bool)
    for seed in PERTURB_SEEDS:
        moved |= twin(pool_name, variant, perturb=seed, **extra)["iters"] != base
    return tuple(int(b) for b in np.flatnonzero(moved))


def full_solve_runs():
    """every (pool, variant) of layer B's full solves on the pools that solve (the stalled pool's sets end on plateaus and
    limits: its counts are held to the bound without exception)"""
    return [(p, v) for p in LAYER_B for v in ("defaults",) + LAYER_B[p]]


# ---- problems whose status at an iteration limit hangs on the deciding threshold -------------------------------------
# {(pool, variant, limit of layer A or None): indices}: the twin ends them 2 or 5 and gives another status with
# inaccurate_floor -- for a floor of 0 eps_abs = eps_rel -- halved or doubled.  On every route they must still end 2 or 5.
# tests/test_options_cases.py holds the table to exactly what the twin does, and to a tenth of a pool.
DROPPED = {
    ("stalled", "noretry_floor0", None): (0,),
    ("n8_soc", "short100_floor_default", None): (17, 19),
    ("n8_soc", "retry2_140", None): (4, 18),
    ("n8_soc", "retry2_400", None): (4, 18),
    ("n8_soc", "retry1_400", None): (4, 18),
    ("n8_soc", "retry_stall0", None): (4, 18),
    ("n8_soc", "retry_rho0.5", None): (18,),
}


def base_of(limit):
    """the options every run of a layer shares: layer A with its iteration limit, layer B for ``None``"""
    return dict(LAYER_B_BASE) if limit is None else dict(LAYER_A_BASE, max_iter=int(limit))


def dropped(pool_name, variant, limit=None):
    return tuple(DROPPED.get((pool_name, variant, limit), ()))


def limit_runs():
    """every (pool, variant, limit) of the GPU tests in which a problem may end at an iteration limit or on a plateau"""
    runs = [(p, v, m) for p in LAYER_A for v, m in layer_a_runs(p)]
    runs += [("stalled", v, None) for v in ("defaults",) + STALL_SETS]
    runs += [("n8_soc", v, None) for v in FLOOR_SETS + RETRY_SETS]
    return runs


# ---- the twin -------------------------------------------------------------------------------------------------------
_TWIN_KEYS = ("eps_abs", "eps_rel", "rho", "sigma", "alpha", "adapt_tol", "reg_rel", "max_iter", "check_every", "adapt_every",
              "accel_mem", "stall_iters", "retry_passes", "retry_max_iter", "retry_rho", "inaccurate_floor")


def options_of(variant, **extra):
    """keywords of ``backend.default_options``: the variant's set with ``extra`` on top"""
    kw = dict(VARIANTS[variant])
    kw.update(extra)
    return kw


@functools.lru_cache(maxsize=None)
def _twin(pool_name, variant, t_max, k, extra):
    import copy

    from oracle import admm_port

    kw = options_of(variant, **dict(extra))
    kw.pop("polish_iters", None)   # (the twin has no polish)
    seed = kw.pop("perturb", None)
    assert set(kw) <= set(_TWIN_KEYS), kw
    kw.setdefault("accel_mem", 0)
    batch = H.pad_batch(pool(pool_name), t_max, k)
    if seed is not None:   # the cost vector moved by PERTURB relative, entry by entry
        batch = copy.copy(batch)
        batch.q = batch.q * (1.0 + PERTURB * np.random.default_rng(seed).standard_normal(batch.q.shape))
    out = admm_port.solve_batch(batch, threads=min(16, admm_port.max_threads()), **kw)
    for a in out.values():
        a.setflags(write=False)
    return out


def twin(pool_name, variant, t_max=None, k=None, **extra):
    """oracle/admm_port.solve_batch of the pool padded to (t_max, k) (default: its own shape) under the variant's options
    with ``extra`` on top; cached, read-only"""
    p = pool(pool_name)
    return _twin(pool_name, variant, int(t_max or p.Tm), int(k or p.K), tuple(sorted(extra.items())))


def threshold_scaled(variant, factor, **extra):
    """``extra`` with the threshold that decides between MAX_ITER and SOLVED_INACCURATE scaled: inaccurate_floor, or for a
    floor of 0 eps_abs = eps_rel"""
    kw = options_of(variant, **extra)
    floor = kw.get("inaccurate_floor", 1e-5)
    out = dict(extra)
    if floor > 0:
        out["inaccurate_floor"] = floor * factor
    else:
        out["eps_abs"] = kw.get("eps_abs", 1e-8) * factor
        out["eps_rel"] = kw.get("eps_rel", 1e-8) * factor
    return out


def fragile(pool_name, variant, **extra):
    """indices whose twin status is 2 or 5 and changes with the deciding threshold halved or doubled"""
    base = twin(pool_name, variant, **extra)["status"]
    same = np.ones(len(base), bool)
    for f in (0.5, 2.0):
        same &= twin(pool_name, variant, **threshold_scaled(variant, f, **extra))["status"] == base
    return tuple(int(b) for b in np.flatnonzero(~same & np.isin(base, (2, 5))))
