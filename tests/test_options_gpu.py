"""Every kernel route under solver options other than the defaults, against oracle/admm_port under the same options
(tests/options_cases.py: pools, option sets, tolerances; tests/test_options_cases.py: the twin tells every set apart).

Each pool is padded to the smallest shape of each kernel family it reaches and launched through the device entry with
every output poisoned, once per (family, option set).  The twin is run at the pool's own shape and its answer padded:
dead periods and empty slots change none of its bits (tests/test_options_cases.py::test_padding_leaves_the_twin_alone).

  A  truncated trajectories (no Anderson columns, polish or retry; a limit of three check periods): iteration count and
     status of the twin, every output written, dead periods zero, iterate, multipliers and residuals at TRAJ_TOL;
  B  full solves (no Anderson columns, no polish): the twin's status, the certificate of oracle/kkt.py, the twin's
     iteration count within one check period (but for the problems of options_cases.ITER_FRAGILE, whose count the twin
     itself does not hold under a 1e-13 perturbation); the stall, retry and floor sets;
  C  as shipped (Anderson columns, polish) at check periods 7 and 1; the polish hand-over at period 7;
  then what acnqp_solve_batch refuses and accepts, and that the Python surface passes ``solver_options`` on."""
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests import options_cases as OC

FAMILIES = {"wave1", "wave2", "wave3", "wave4", "wave5", "tiled_ct1", "tiled_ct2", "long_lds", "long_ws", "stream", "general"}


@functools.lru_cache(maxsize=None)
def _site(pool):
    """(handle, {family: (t_max, k_sessions)}) of a pool; the handle stays open for the module"""
    from adacharge_amd.backend import SiteHandle

    batch = OC.pool(pool)
    h = SiteHandle(batch.site, 0)
    want = OC.POOLS[pool]
    shapes = {f: s for f, s in H.route_shapes(h, batch).items() if want is None or f in want}
    for fam, (t, k) in shapes.items():
        assert h.route(t, k, batch.B)[0] == fam
    return h, shapes


@functools.lru_cache(maxsize=None)
def _padded(pool, shape):
    return H.pad_batch(OC.pool(pool), *shape)


def _options(variant, limit, **extra):
    from adacharge_amd.backend import default_options

    return default_options(**OC.options_of(variant, **dict(OC.base_of(limit), **extra)))


@functools.lru_cache(maxsize=None)
def _run(pool, variant, limit=None):
    """{family: outputs} of one option set in layer A (``limit``) or B (None): one poisoned launch per family"""
    h, shapes = _site(pool)
    return {fam: H.launch_poisoned(h, _padded(pool, shape), _options(variant, limit)) for fam, shape in shapes.items()}


def _twin(pool, variant, t_max, limit=None, **extra):
    """the twin's answer at the pool's own shape, x and y padded to ``t_max`` periods"""
    own = OC.twin(pool, variant, **dict(OC.base_of(limit), **extra))
    return dict(own, x=H.pad_result(own["x"], t_max), y=H.pad_result(own["y"], t_max))


def _written(out, where):
    for key in ("x", "y", "pri_res", "dua_res", "obj"):
        assert not np.isnan(out[key]).any(), f"{where}: {key} left unwritten"
    assert (out["iters"] >= 0).all() and (out["status"] > 0).all(), f"{where}: iters / status left unwritten"


def _dead_periods_zero(batch, out, where):
    for b in range(batch.B):
        T = int(batch.T[b])
        assert not out["x"][b][:, T:].any() and not out["y"][b][:, T:].any(), f"{where}: problem {b} dead periods"


def _status_as_the_twin(out, twin, skip, where):
    keep = np.ones(len(twin["status"]), bool)
    keep[list(skip)] = False
    assert np.array_equal(out["status"][keep], twin["status"][keep]), (where, out["status"], twin["status"])
    assert np.isin(out["status"][~keep], (2, 5)).all(), (where, skip, out["status"])   # (on the line between 2 and 5)


def _certified(padded, out, status_limits, options, where):
    """every answer the kernel calls SOLVED passes the certificate at the limits of ``status_limits``"""
    for b in np.flatnonzero(out["status"] == 1):
        obj = out["obj"][b] + kkt.prox_terms(padded, b, out["x"][b])
        bad = kkt.failures(kkt.certify(padded, b, out["x"][b], out["y"][b], obj, options=options), status_limits)
        assert not bad, f"{where}: problem {b} (iters {int(out['iters'][b])}): {bad}"


# ---- A: truncated trajectories ------------------------------------------------------------------------------------------
def _rel(a, b, floor):
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("pool", list(OC.LAYER_A))
def test_layer_a_truncated_trajectories_follow_the_twin(pool):
    batch = OC.pool(pool)
    _, shapes = _site(pool)
    worst, failed = {}, []
    for variant, limit in OC.layer_a_runs(pool):
        for fam, out in _run(pool, variant, limit).items():
            t, k = shapes[fam]
            where = f"{pool} on {fam} (t_max {t}, K {k}), {variant} at limit {limit}"
            twin = _twin(pool, variant, t, limit)
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            at_limit = twin["iters"] == limit
            assert np.array_equal(out["iters"][at_limit], twin["iters"][at_limit]), (where, out["iters"], twin["iters"])
            assert (np.abs(out["iters"] - twin["iters"])[~at_limit] <= OC.check_period(variant)).all(), (where, out["iters"], twin["iters"])
            _status_as_the_twin(out, twin, OC.dropped(pool, variant, limit), where)
            same = out["iters"] == twin["iters"]   # (a problem that converged a check earlier or later is another iterate)
            assert same.mean() >= 0.9, (where, out["iters"], twin["iters"])
            # x in A; y relative to max(1, |y_twin|_inf) of the problem; the residuals of a problem the twin leaves unsolved
            # relative to their own value (a SOLVED one's are roundoff below eps on either side: its status says so)
            dx = float(np.abs(out["x"] - twin["x"])[same].max())
            ymag = np.maximum(1.0, np.abs(twin["y"]).reshape(batch.B, -1).max(axis=1))[:, None, None]
            dy = float((np.abs(out["y"] - twin["y"]) / ymag)[same].max())
            live = same & (twin["status"] != 1)
            dr = max(_rel(out[key][live], twin[key][live], 1e-300) for key in ("pri_res", "dua_res")) if live.any() else 0.0
            w = worst.setdefault(fam, dict(floor=0.0, x=0.0, y=0.0, res=0.0))
            if variant == "defaults":
                w["floor"] = max(w["floor"], dx)
            w["x"], w["y"], w["res"] = max(w["x"], dx), max(w["y"], dy), max(w["res"], dr)
            if dx > OC.TRAJ_TOL or dy > OC.TRAJ_Y_REL or dr > OC.TRAJ_RES_REL:
                failed.append((where, dx, dy, dr))
    for fam, w in sorted(worst.items()):
        print(f"[options] A {pool} on {fam}: |x - x_twin| {w['floor']:.2e} A at the defaults, {w['x']:.2e} A over all sets; "
              f"y {w['y']:.2e}, residuals {w['res']:.2e} (relative)")
    assert not failed, failed


@pytest.mark.gpu
def test_layer_a_reaches_every_family():
    reached = set()
    for pool in OC.LAYER_A:
        reached |= set(_site(pool)[1])
    assert reached == FAMILIES, sorted(FAMILIES - reached)


# ---- B: full solves -----------------------------------------------------------------------------------------------------
def _iteration_differences(out, twin, variant, passes, where, failed, fragile=()):
    """worst |iters - iters_twin| over the problems held to the bound (all but ``fragile``, options_cases.ITER_FRAGILE)"""
    d = np.abs(out["iters"] - twin["iters"])
    d[list(fragile)] = 0
    bound = OC.ITER_BOUND_PERIODS * OC.check_period(variant) * passes
    if (d > bound).any():
        failed.append((where, bound, {int(b): (int(out["iters"][b]), int(twin["iters"][b])) for b in np.flatnonzero(d > bound)}))
    return int(d.max())


@pytest.mark.gpu
@pytest.mark.parametrize("pool", list(OC.LAYER_B))
def test_layer_b_full_solves_follow_the_twin(pool):
    batch = OC.pool(pool)
    _, shapes = _site(pool)
    worst, failed = {}, []
    for variant in ("defaults",) + OC.LAYER_B[pool]:
        opts = _options(variant, None)
        for fam, out in _run(pool, variant).items():
            t, k = shapes[fam]
            where = f"{pool} on {fam} (t_max {t}, K {k}), {variant}"
            twin = _twin(pool, variant, t)
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            assert (twin["status"] == 1).all(), (where, twin["status"])
            assert np.array_equal(out["status"], twin["status"]), (where, out["status"])
            # the certificate's limits were set from the twin at eps = 1e-8 and scale with eps: an answer at eps = 1e-5 owes
            # what SOLVED_INACCURATE owes (1e3 times the SOLVED limits); one at 1e-10 the SOLVED limits
            _certified(_padded(pool, (t, k)), out, kkt.ST_SOLVED_INACCURATE if variant == "eps1e-5" else kkt.ST_SOLVED, opts, where)
            d = _iteration_differences(out, twin, variant, 1, where, failed, OC.ITER_FRAGILE.get((pool, variant), ()))
            w = worst.setdefault(fam, [0, 0])
            w[0 if variant == "defaults" else 1] = max(w[0 if variant == "defaults" else 1], d)
            if OC.VARIANTS[variant].get("adapt_every") == 0:
                # a fixed penalty: nothing adapts, so nothing can flip -- the twin's count -- and no retry pass runs
                assert np.array_equal(out["iters"], twin["iters"]), (where, out["iters"], twin["iters"])
                assert (out["iters"] <= opts.max_iter).all(), where
            if pool == "ct54_lp":
                dx = float(np.abs(out["x"] - twin["x"]).max())
                assert dx <= OC.RATE_TOL, (where, dx)
    for fam, (d0, d1) in sorted(worst.items()):
        print(f"[options] B {pool} on {fam}: worst |iters - iters_twin| {d0} at the defaults, {d1} over the other sets (ITER_FRAGILE aside)")
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ("defaults",) + OC.STALL_SETS)
def test_stall_and_retry_sets_on_the_stalled_pool(variant):
    """ten congested problems that end a pass on a plateau: the stall window, the retry passes and the floor decide status
    and count -- the twin's, within one check period per pass that can run"""
    batch = OC.pool("stalled")
    _, shapes = _site("stalled")
    failed = []
    passes = 1 + int(OC.VARIANTS[variant].get("retry_passes", 2))
    for fam, out in _run("stalled", variant).items():
        t, k = shapes[fam]
        where = f"stalled on {fam} (t_max {t}, K {k}), {variant}"
        twin = _twin("stalled", variant, t)
        _written(out, where)
        _dead_periods_zero(batch, out, where)
        print(f"[options] B {where}: statuses {np.bincount(out['status'], minlength=6).tolist()}, worst |iters - iters_twin| "
              f"{int(np.abs(out['iters'] - twin['iters']).max())}")
        _status_as_the_twin(out, twin, OC.dropped("stalled", variant), where)
        _certified(_padded("stalled", (t, k)), out, kkt.ST_SOLVED, _options(variant, None), where)
        _iteration_differences(out, twin, variant, passes, where, failed)
    assert not failed, failed


@pytest.mark.gpu
def test_floor_and_retry_sets_under_a_short_limit():
    """n8_soc: the floor decides between MAX_ITER and SOLVED_INACCURATE after 100 iterations; after 240, what is unsolved
    is retried as retry_passes, retry_max_iter and stall_iters say -- the totals 380, 480 and 720 on exactly the twin's
    problems, none with the stall window off, none with a fixed penalty; and retry_rho shows in the kept iterate."""
    batch = OC.pool("n8_soc")
    _, shapes = _site("n8_soc")
    worst = 0.0
    for variant in OC.FLOOR_SETS + OC.RETRY_SETS:
        for fam, out in _run("n8_soc", variant).items():
            t, k = shapes[fam]
            where = f"n8_soc on {fam} (t_max {t}, K {k}), {variant}"
            twin = _twin("n8_soc", variant, t)
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            _status_as_the_twin(out, twin, OC.dropped("n8_soc", variant), where)
            # every pass of an unsolved problem runs to its limit: the totals are exact; a solved one within a check period
            unsolved = twin["status"] != 1
            assert np.array_equal(out["iters"][unsolved], twin["iters"][unsolved]), (where, out["iters"], twin["iters"])
            assert (np.abs(out["iters"] - twin["iters"]) <= 20).all(), (where, out["iters"], twin["iters"])
            if variant in ("retry_stall0", "fixed_no_retry"):
                assert (out["iters"] <= 240).all(), (where, out["iters"])
            if variant.startswith("retry_rho"):
                assert (out["status"] == 5).all() and (out["iters"] > 240).all(), (where, out["status"], out["iters"])
                dx = float(np.abs(out["x"] - twin["x"]).max())
                worst = max(worst, dx)
                assert dx <= OC.TRAJ_TOL, (where, dx)
    print(f"[options] B n8_soc, retry_rho sets: worst |x - x_twin| {worst:.2e} A")


# ---- C: as shipped ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pool", ["n8_soc", "pods18_lin", "wide80_soc", "n2_t40_lin"])
def test_layer_c_anderson_against_an_odd_check_period(pool):
    """check_every 7 and 1 with Anderson events every 5 iterations and the polish on, through to the end"""
    from adacharge_amd.backend import default_options

    batch = OC.pool(pool)
    h, shapes = _site(pool)
    for variant in OC.LAYER_C:
        opts = default_options(**OC.VARIANTS[variant])
        ce = OC.check_period(variant)
        for fam, (t, k) in shapes.items():
            where = f"{pool} on {fam} (t_max {t}, K {k}), {variant}"
            padded = _padded(pool, (t, k))
            out = H.launch_poisoned(h, padded, opts)
            own = OC.twin(pool, variant, accel_mem=h.accel_columns(t, k, opts))
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            assert (own["status"] == 1).all() and (out["status"] == 1).all(), (where, out["status"], own["status"])
            _certified(padded, out, kkt.ST_SOLVED, opts, where)
            dx = float(np.abs(out["x"] - H.pad_result(own["x"], t)).max())
            print(f"[options] C {where}: worst |x - x_twin| {dx:.2e} A, iterations {int(out['iters'].min())} ... {int(out['iters'].max())} "
                  f"(twin {int(own['iters'].min())} ... {int(own['iters'].max())})")
            assert dx <= OC.RATE_TOL, (where, dx)
            assert ((out["iters"] % ce == 0) | (out["iters"] == opts.max_iter)).all(), (where, out["iters"])


@pytest.mark.gpu
def test_polish_hand_over_at_an_odd_check_period():
    """the stalled pool at check_every = 7, defaults otherwise: polish_iters = 800 is handed over at 798, the polish solves"""
    from adacharge_amd.backend import default_options

    h, shapes = _site("stalled")
    batch = OC.pool("stalled")
    opts = default_options(check_every=7)
    polishing = {fam: s for fam, s in shapes.items() if h.route(*s, batch.B)[1]}
    assert polishing, shapes
    for fam, (t, k) in polishing.items():
        where = f"stalled on {fam} (t_max {t}, K {k}), check_every 7"
        padded = _padded("stalled", (t, k))
        before = h.polish_stats()
        out = H.launch_poisoned(h, padded, opts)
        after = h.polish_stats()
        print(f"[options] C {where}: polish solved {after['solved'] - before['solved']} of {after['attempted'] - before['attempted']}, "
              f"iterations {out['iters'].tolist()}")
        _written(out, where)
        assert after["solved"] > before["solved"], (where, before, after)
        assert (out["status"] == 1).all(), (where, out["status"])
        _certified(padded, out, kkt.ST_SOLVED, opts, where)


# ---- refusals -----------------------------------------------------------------------------------------------------------
REFUSED = (dict(eps_abs=float("nan")), dict(eps_rel=-1.0), dict(max_iter=0), dict(check_every=0), dict(rho=0.0), dict(sigma=-1.0),
           dict(alpha=0.0), dict(alpha=2.0), dict(adapt_tol=1.0), dict(reg_rel=-1.0), dict(adapt_every=-1), dict(polish_iters=-1),
           dict(stall_iters=-1), dict(retry_passes=9), dict(retry_max_iter=0), dict(retry_rho=0.0), dict(inaccurate_floor=-1.0))
ACCEPTED = (dict(eps_abs=0.0), dict(sigma=0.0), dict(adapt_every=0), dict(stall_iters=0), dict(retry_passes=8), dict(inaccurate_floor=0.0))


@pytest.mark.gpu
def test_bad_option_values_are_refused_before_any_device_work():
    import torch
    from adacharge_amd.backend import default_options, load_library

    h, _ = _site("n8_soc")
    four = OC.pool("n8_soc").subset(slice(0, 4))
    for kw in REFUSED:
        opts = default_options(**kw)
        with pytest.raises(ValueError, match="invalid option value"):
            h.solve(four, opts)
        assert "invalid option value" in load_library().acnqp_last_error().decode(), kw
        dev = H.poisoned_device_batch(four)
        with pytest.raises(ValueError, match="invalid option value"):
            h.solve_device(dev, opts, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = H.device_outputs(dev)
        for key in ("x", "y", "pri_res", "dua_res", "obj"):
            assert np.isnan(out[key]).all(), (kw, key)
        assert (out["iters"] == -1).all() and (out["status"] == -1).all(), (kw, out["iters"], out["status"])


@pytest.mark.gpu
def test_boundary_option_values_are_accepted():
    from adacharge_amd.backend import default_options

    h, _ = _site("n8_soc")
    four = OC.pool("n8_soc").subset(slice(0, 4))
    for kw in ACCEPTED:
        opts = default_options(**kw)
        assert opts.eps_rel > 0
        out = H.launch_poisoned(h, four, opts)
        _written(out, kw)
        assert (out["status"] == 1).all(), (kw, out["status"])
        _certified(four, out, kkt.ST_SOLVED, opts, str(kw))


# ---- the Python surface passes the options on -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_solver_options_reach_the_library():
    from adacharge_amd import AdaptiveChargingOptimization
    from adacharge_amd.backend import SiteHandle, default_options
    from tests import verdict_cases as V

    infra, iface, obj, _ = V._context("n8", "SOC")
    sessions = V.feeder_equalities("n8", "SOC", -0.3).sessions
    kw = dict(alpha=1.0, check_every=7, adapt_every=7)
    opt = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", enforce_energy_equality=True, solver_options=kw)
    opt.solve_batch([sessions], infra)   # (solve() asks for tighter residuals on top: _SINGLE_DEFAULTS)
    res, batch = opt.last_result, opt.last_batch
    h = SiteHandle(batch.site, 0)
    own = h.solve(batch, default_options(**kw), want_y=True)
    h.close()
    for key in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj"):
        assert np.array_equal(getattr(res, key), getattr(own, key)), key
    assert int(own.status[0]) == 1 and int(own.iters[0]) % 7 == 0, (own.status, own.iters)
