"""Warm-started solves: the pools, the kinds of warm point and the CPU reference of tests/test_warm_cases.py (the reference
alone: padding, every kind told apart, oracle/admm_ref grounds the twin's warm start, stale entries) and
tests/test_warm_gpu.py (every kernel route follows the twin from every kind of warm point).  A plain module, like
options_cases.py.

Each of the five solver kernels has its own copy of the warm start (include/acn_qp.h: z = Proj(warm_x), y2 = warm_y read
through the kernel's own row map and row scaling, y1 = -(P z + q + G' y2)).  A warm start taken wrongly still converges, so
"fewer iterations, answer near the cold one" does not see it; the iterate one step and sixty steps from the start point does.

Kinds (built from the twin's cold answer (x*, y*) at eps = 1e-10, fixed seed):
  exact      (x*, y*)
  zero       both arrays zero (given, so the warm path runs: not the cold start -1e5 q)
  shifted    both arrays one period earlier, zero in the last period -- what a closed-loop caller passes
  perturbed  x* U(0.5, 1.5) with U(-5, 40) outside every window, at dead periods and in the padding beyond the pool's Tm;
             y* U(0.5, 1.5), a tenth of the zero multipliers U(0, 1), a tenth of the live LINEAR and peak multipliers negated
  stale      exact, with U(-3, 3) in warm_y at every t >= horizon[b], padding included: the library reads those as zero
"""
import functools
import zlib

import numpy as np

from tests import helpers as H
from tests import options_cases as OC

# ---- pools ----------------------------------------------------------------------------------------------------------
# name -> kernel families to launch (None: every family the pool reaches).  Between them all eleven.  The four row pools
# bring every row type into warm_y: SOC pairs and a peak row (scalar, vector and unlimited), LINEAR rows and a peak row under
# energy equalities, 28 SOC rows and a peak row (the padded rows of two row tiles), the flat row and the max row.
MIXED = ("ct54_soc_mixed", "ct54_lin_eq_mixed")   # horizons 12 / 10 / 8 in one batch: dead periods inside Tm
ROW_POOLS = MIXED + ("n60_t17_soc_peak", "n100_t24_lf", "jpl_t28_dc")
POOLS = {name: OC.POOLS[name] for name in ("n8_soc", "pods18_lin", "wide80_soc", "n2_t40_lin")}
POOLS.update({name: None for name in ROW_POOLS})
SEED = 20240


@functools.lru_cache(maxsize=None)
def pool(name):
    if name in OC.POOLS:
        return OC.pool(name)
    if name == "ct54_soc_mixed":
        return H.certificate_pool("caltech54", "SOC", 12, 24, 32, two=False, peak="mixed")
    if name == "ct54_lin_eq_mixed":
        return H.certificate_pool("caltech54", "LINEAR", 12, 24, 34, eq=True, two=False, peak="mixed")
    seeds = {"n60_t17_soc_peak": 42, "n100_t24_lf": 44, "jpl_t28_dc": 45}
    return H.edges_pool(name, 24, seeds[name])


# ---- option sets of the runs ----------------------------------------------------------------------------------------
RUNS = {
    "one": dict(OC.LAYER_A_BASE, max_iter=1, check_every=1, adapt_every=0),   # the iterate one step from the start point
    "m20": dict(OC.LAYER_A_BASE, max_iter=20),
    "m60": dict(OC.LAYER_A_BASE, max_iter=60),
    "plain": dict(accel_mem=0),                  # default options but for the Anderson columns
    "full": dict(OC.LAYER_B_BASE),               # ... and no polish (a warm-started launch takes none anyway)
    "retry": dict(OC.LAYER_B_BASE, **OC.VARIANTS["stall200_retry1"]),   # pass 0 starts warm, the retry starts cold
    "shipped": {},
}
LAYER_A = ("one", "m60")
STALE_RUNS = ("one", "m20", "m60")
KINDS = ("exact", "zero", "shifted", "perturbed")


def check_period(run):
    return int(RUNS[run].get("check_every", 20))


def kinds_of(name, t_max=None):
    """the kinds a pool is launched from at ``t_max`` periods: ``stale`` where there is a dead period to write to"""
    p = pool(name)
    return KINDS + (("stale",) if name in MIXED or (t_max or p.Tm) > p.Tm else ())


# ---- warm points ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cold_answer(name):
    """the twin's cold answer at eps = 1e-10, no Anderson columns: (x*, y*), read-only"""
    from oracle import admm_port

    out = admm_port.solve_batch(pool(name), threads=min(16, admm_port.max_threads()), eps_abs=1e-10, eps_rel=1e-10, accel_mem=0)
    assert np.isin(out["status"], (1, 5)).all() and (name == "stalled" or (out["status"] == 1).all()), (name, out["status"])
    for a in out.values():
        a.setflags(write=False)
    return out


def _rng(name, kind, part):
    return np.random.default_rng([SEED, zlib.crc32(name.encode()), zlib.crc32(kind.encode()), part])


def masks(batch, t_max):
    """(inside a session window (B, N, t_max), live period (B, 1, t_max))"""
    t = np.arange(t_max)
    win = np.zeros((batch.B, batch.N, t_max), bool)
    for k in range(batch.K):
        off, ln = batch.s_off[:, k, :, None], batch.s_len[:, k, :, None]
        win |= (t >= off) & (t < off + ln)
    live = (t[None, :] < np.asarray(batch.T)[:, None])[:, None, :]
    return win & live, live


@functools.lru_cache(maxsize=None)
def warm(name, kind, t_max=None):
    """(warm_x (B, N, t_max), warm_y (B, Mg, t_max)) of a kind, read-only; ``t_max`` defaults to the pool's own Tm.  The part
    inside the pool's own shape is the same at every ``t_max``."""
    batch = pool(name)
    Tm = batch.Tm
    t_max = int(t_max or Tm)
    site = batch.site
    xs, ys = cold_answer(name)["x"], cold_answer(name)["y"]
    win, live = masks(batch, Tm)
    if kind in ("exact", "stale"):
        x0, y0 = xs.copy(), ys.copy()
    elif kind == "zero":
        x0, y0 = np.zeros_like(xs), np.zeros_like(ys)
    elif kind == "shifted":
        x0, y0 = np.zeros_like(xs), np.zeros_like(ys)
        x0[..., :-1], y0[..., :-1] = xs[..., 1:], ys[..., 1:]
    elif kind == "perturbed":
        r = _rng(name, kind, 0)
        x0 = xs * r.uniform(0.5, 1.5, xs.shape)
        x0 = np.where(win, x0, r.uniform(-5.0, 40.0, xs.shape))
        y0 = ys * r.uniform(0.5, 1.5, ys.shape)
        y0 = np.where((ys == 0) & (r.uniform(size=ys.shape) < 0.1), r.uniform(0.0, 1.0, ys.shape), y0)
        signed = np.zeros(site.Mg, bool)   # rows whose multiplier has a sign: LINEAR rows and the peak row
        if int(site.cone) == 0:
            signed[: site.M] = True
        if site.has_peak:
            signed[site.Mg - 1] = True
        y0 = np.where(signed[None, :, None] & (r.uniform(size=ys.shape) < 0.1), -y0, y0)
        y0 = y0 * live
    else:
        raise KeyError(kind)
    x0, y0 = H.pad_result(x0, t_max), H.pad_result(y0, t_max)
    _, live_p = masks(batch, t_max)
    if kind == "perturbed" and t_max > Tm:
        x0[..., Tm:] = _rng(name, kind, 1).uniform(-5.0, 40.0, x0[..., Tm:].shape)
    if kind == "stale":
        junk = np.zeros_like(y0)
        junk[..., :Tm] = _rng(name, kind, 0).uniform(-3.0, 3.0, ys.shape)
        junk[..., Tm:] = _rng(name, kind, 1).uniform(-3.0, 3.0, y0[..., Tm:].shape)
        y0 = np.where(live_p, y0, junk)
    if kind != "stale":
        assert not (y0 * ~live_p).any()
    x0.setflags(write=False)
    y0.setflags(write=False)
    return x0, y0


# ---- the twin -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _twin(name, kind, run, t_max, k, extra):
    import copy

    from oracle import admm_port

    kw = dict(RUNS[run])
    kw.update(dict(extra))
    kw.pop("polish_iters", None)   # (the twin has no polish)
    seed = kw.pop("perturb", None)
    assert set(kw) <= set(OC._TWIN_KEYS), kw
    kw.setdefault("accel_mem", 0)
    batch = H.pad_batch(pool(name), t_max, k)
    if seed is not None:   # the cost vector moved by OC.PERTURB relative, entry by entry
        batch = copy.copy(batch)
        batch.q = batch.q * (1.0 + OC.PERTURB * np.random.default_rng(seed).standard_normal(batch.q.shape))
    if kind != "cold":
        kw["warm_x"], kw["warm_y"] = warm(name, kind, t_max)
    out = admm_port.solve_batch(batch, threads=min(16, admm_port.max_threads()), **kw)
    for a in out.values():
        a.setflags(write=False)
    return out


def twin(name, kind, run, t_max=None, k=None, **extra):
    """oracle/admm_port.solve_batch of the pool padded to (t_max, k) (default: its own shape) from the warm point ``kind``
    (``"cold"``: none) under RUNS[run] with ``extra`` on top; cached, read-only"""
    p = pool(name)
    return _twin(name, kind, run, int(t_max or p.Tm), int(k or p.K), tuple(sorted(extra.items())))


def twin_padded(name, kind, run, t_max, **extra):
    """the twin's answer at the pool's own shape, x and y padded to ``t_max`` periods.  A pool with a max row is solved at
    ``t_max`` instead: the demand-charge prox is a Newton iteration over all t_max periods, whose first steps the dead ones
    enter (tau < 0), so padding moves the twin by roundoff there (tests/test_warm_cases.py) -- and a kernel launched at
    ``t_max`` does the same."""
    own = twin(name, kind, run, t_max if getattr(pool(name).site, "has_max", False) else None, **extra)
    return dict(own, x=H.pad_result(own["x"], t_max), y=H.pad_result(own["y"], t_max))


def fragile(name, kind, run):
    """indices whose twin status is 2 or 5 and changes with the deciding threshold halved or doubled (OC.fragile)"""
    base = twin(name, kind, run)["status"]
    floor = RUNS[run].get("inaccurate_floor", 1e-5)
    same = np.ones(len(base), bool)
    for f in (0.5, 2.0):
        same &= twin(name, kind, run, inaccurate_floor=floor * f)["status"] == base
    return tuple(int(b) for b in np.flatnonzero(~same & np.isin(base, (2, 5))))


def iter_fragile(name, kind, run="full"):
    """indices whose iteration count the twin itself moves when the cost vector moves by OC.PERTURB (OC.iter_fragile)"""
    base = twin(name, kind, run)["iters"]
    moved = np.zeros(len(base), bool)
    for seed in OC.PERTURB_SEEDS:
        moved |= twin(name, kind, run, perturb=seed)["iters"] != base
    return tuple(int(b) for b in np.flatnonzero(moved))


# ---- measured ---------------------------------------------------------------------------------------------------------
# {(pool, kind): indices}: OC.ITER_FRAGILE for the full solves of layer C; tests/test_warm_cases.py holds it to the twin.
ITER_FRAGILE = {("wide80_soc", "perturbed"): (18,), ("wide80_soc", "shifted"): (18,)}
FULL_KINDS = ("perturbed", "shifted")
# the twin's own move from ``exact`` under default options (no Anderson columns): |x - x*|_inf of a pool in A, rounded up
# (tests/test_warm_cases.py holds the figures to what the twin does)
EXACT_MOVE = {"n8_soc": 5.4e-8, "pods18_lin": 5.3e-8, "wide80_soc": 5.8e-8, "n2_t40_lin": 1.32e-7, "ct54_soc_mixed": 8.9e-7,
              "ct54_lin_eq_mixed": 3.2e-7, "n60_t17_soc_peak": 3.3e-8, "n100_t24_lf": 3.7e-6, "jpl_t28_dc": 3.3e-8}
# the stalled pool under stall200_retry1 from ``perturbed``: problems whose status (2 or 5) hangs on the deciding threshold
# (options_cases.DROPPED; the twin gives another status with inaccurate_floor halved or doubled) -- two of the ten
RETRY_DROPPED = (6, 8)
# Layer A of tests/test_warm_gpu.py, measured on an MI355X: route -> worst |x - x_twin| in A over every pool, kind and both
# limits.  Every route stays under the cold-start tolerances of options_cases.py (TRAJ_TOL 5.3e-8 A) by a factor of forty
# or more, the large-site kernel included: it needs no constant of its own here.  The three routes above 1e-9 A owe it to
# n100_t24_lf alone (the flat row's prox; elsewhere they are at 2.4e-11 A or below); y relative to max(1, |y_twin|_inf) is at
# most 3.2e-12 (n100_t24_lf; elsewhere 1.1e-13), the residuals of an unsolved problem relative to themselves 1.5e-10.
WARM_MEASURED = {
    "wave1": 9.19e-12, "wave2": 9.19e-12, "wave3": 2.03e-11, "wave4": 2.03e-11, "wave5": 9.19e-12, "tiled_ct1": 2.41e-11,
    "tiled_ct2": 2.09e-11, "long_lds": 2.42e-11, "long_ws": 1.31e-09, "stream": 1.10e-09, "general": 1.07e-09,
}
