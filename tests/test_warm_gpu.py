"""Every kernel route from a warm point, against oracle/admm_port from the same point (tests/warm_cases.py: pools, kinds of
warm point, the twin; tests/test_warm_cases.py: the twin tells every kind apart and oracle/admm_ref grounds its warm start).

Each of the five solver kernels loads warm_x and warm_y for itself: warm_y through its own row map and row scaling, and
y1 = -(P z + q + G' y2) with its own G'y product.  Each pool is padded to the smallest shape of each kernel family it
reaches and launched through the device entry with every output poisoned, once per (family, kind, limit).

  A  truncated trajectories (no Anderson columns, polish or retry) after 1 and after 60 iterations: status and iteration
     count of the twin, every output written, dead periods zero, iterate, multipliers and residuals at the tolerances
     options_cases.py measured on cold starts;
  B  from ``exact`` under default options (no Anderson columns), without the twin: SOLVED at the first check, at most ten
     times the twin's own move away from (x*, y*);
  C  full solves from ``perturbed`` and ``shifted``: the twin's status and count, the certificate of oracle/kkt.py; as
     shipped: SOLVED, certified, the cold answer, and no polish behind a warm start;
  D  a retry pass behind a warm pass 0 on the stalled pool;
  E  warm_y entries at dead periods are read as zero."""
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests import options_cases as OC
from tests import warm_cases as WC
from tests.test_options_gpu import (FAMILIES, _certified, _dead_periods_zero, _iteration_differences, _rel, _status_as_the_twin,
                                    _written)

OUTPUTS = ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")
WORST = {}   # route -> worst |x - x_twin| of layer A in this session


@functools.lru_cache(maxsize=None)
def _site(name):
    """(handle, {family: (t_max, k_sessions)}) of a pool; the handle stays open for the module"""
    from adacharge_amd.backend import SiteHandle

    batch = WC.pool(name)
    h = SiteHandle(batch.site, 0)
    want = WC.POOLS[name] if name in WC.POOLS else OC.POOLS[name]
    shapes = {f: s for f, s in H.route_shapes(h, batch).items() if want is None or f in want}
    for fam, (t, k) in shapes.items():
        assert h.route(t, k, batch.B)[0] == fam
    return h, shapes


@functools.lru_cache(maxsize=None)
def _padded(name, shape):
    return H.pad_batch(WC.pool(name), *shape)


def _options(run):
    from adacharge_amd.backend import default_options

    return default_options(**WC.RUNS[run])


@functools.lru_cache(maxsize=None)
def _launch(name, fam, kind, run):
    """outputs of one poisoned launch of the pool at the family's shape from the warm point ``kind`` (``"cold"``: none)"""
    h, shapes = _site(name)
    warm = None if kind == "cold" else WC.warm(name, kind, shapes[fam][0])
    return H.launch_poisoned(h, _padded(name, shapes[fam]), _options(run), warm=warm)


def _where(name, fam, kind, run):
    t, k = _site(name)[1][fam]
    return f"{name} on {fam} (t_max {t}, K {k}) from {kind}, {run}"


@pytest.mark.gpu
def test_the_pools_reach_every_family():
    reached = set()
    for name in WC.POOLS:
        reached |= set(_site(name)[1])
    assert reached == FAMILIES, sorted(FAMILIES - reached)
    for name in WC.ROW_POOLS + ("n8_soc",):
        assert WC.POOLS[name] is None and len(_site(name)[1]) >= 1


# ---- A: truncated trajectories ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WC.POOLS))
def test_layer_a_truncated_trajectories_follow_the_twin(name):
    batch = WC.pool(name)
    _, shapes = _site(name)
    worst, failed = {}, []
    for run in WC.LAYER_A:
        limit = WC.RUNS[run]["max_iter"]
        for fam, (t, k) in shapes.items():
            for kind in WC.kinds_of(name, t):
                where = _where(name, fam, kind, run)
                out, twin = _launch(name, fam, kind, run), WC.twin_padded(name, kind, run, t)
                _written(out, where)
                _dead_periods_zero(batch, out, where)
                at_limit = twin["iters"] == limit
                assert np.array_equal(out["iters"][at_limit], twin["iters"][at_limit]), (where, out["iters"], twin["iters"])
                assert (np.abs(out["iters"] - twin["iters"])[~at_limit] <= WC.check_period(run)).all(), (where, out["iters"], twin["iters"])
                _status_as_the_twin(out, twin, (), where)
                same = out["iters"] == twin["iters"]
                assert same.mean() >= 0.9, (where, out["iters"], twin["iters"])
                dx = float(np.abs(out["x"] - twin["x"])[same].max())
                ymag = np.maximum(1.0, np.abs(twin["y"]).reshape(batch.B, -1).max(axis=1))[:, None, None]
                dy = float((np.abs(out["y"] - twin["y"]) / ymag)[same].max())
                live = same & (twin["status"] != 1)
                dr = max(_rel(out[key][live], twin[key][live], 1e-300) for key in ("pri_res", "dua_res")) if live.any() else 0.0
                w = worst.setdefault(fam, dict(x=0.0, y=0.0, res=0.0))
                w["x"], w["y"], w["res"] = max(w["x"], dx), max(w["y"], dy), max(w["res"], dr)
                if dx > OC.TRAJ_TOL or dy > OC.TRAJ_Y_REL or dr > OC.TRAJ_RES_REL:
                    failed.append((where, dx, dy, dr))
    for fam, w in sorted(worst.items()):
        WORST[fam] = max(WORST.get(fam, 0.0), w["x"])
        print(f"[warm] A {name} on {fam}: |x - x_twin| {w['x']:.2e} A, y {w['y']:.2e}, residuals {w['res']:.2e} (relative), over all kinds and both limits")
    assert not failed, failed


@pytest.mark.gpu
def test_layer_a_worsts_per_route():
    """the worst |x - x_twin| of a route over the pools run in this session, against WC.WARM_MEASURED (the figures of a whole
    run on an MI355X): ten times the recorded value at the most, and the trajectory tolerance anyway"""
    assert set(WC.WARM_MEASURED) == FAMILIES and max(WC.WARM_MEASURED.values()) <= OC.TRAJ_TOL / 10.0
    for fam, w in sorted(WORST.items()):
        print(f"[warm] A {fam}: worst |x - x_twin| {w:.2e} A (recorded {WC.WARM_MEASURED[fam]:.2e} A)")
        assert w <= 10.0 * WC.WARM_MEASURED[fam], (fam, w)


# ---- B: exact, without the twin -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WC.POOLS))
def test_layer_b_exact_is_done_at_the_first_check(name):
    """From (x*, y*) every route is SOLVED at iters == check_every and has moved at most ten times as far as the twin moves
    itself (capped by RATE_TOL).  A warm_y row read from the wrong ABI row, a missing 1 / rowscale or a wrong sign in y1 is no
    fixed point: it cannot pass, even if the twin shared the mistake."""
    batch = WC.pool(name)
    bound = min(10.0 * WC.EXACT_MOVE[name], OC.RATE_TOL)
    for fam, (t, k) in _site(name)[1].items():
        where = _where(name, fam, "exact", "plain")
        out = _launch(name, fam, "exact", "plain")
        _written(out, where)
        _dead_periods_zero(batch, out, where)
        assert (out["status"] == 1).all() and (out["iters"] == WC.check_period("plain")).all(), (where, out["status"], out["iters"])
        move = float(np.abs(out["x"] - H.pad_result(WC.cold_answer(name)["x"], t)).max())
        print(f"[warm] B {where}: |x - x*| {move:.2e} A (the twin's own move {WC.EXACT_MOVE[name]:.2e} A)")
        assert move <= bound, (where, move, bound)


# ---- C: full solves -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WC.POOLS))
def test_layer_c_full_solves_follow_the_twin(name):
    batch = WC.pool(name)
    failed = []
    for kind in WC.FULL_KINDS:
        for fam, (t, k) in _site(name)[1].items():
            where = _where(name, fam, kind, "full")
            out, twin = _launch(name, fam, kind, "full"), WC.twin_padded(name, kind, "full", t)
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            assert (twin["status"] == 1).all() and np.array_equal(out["status"], twin["status"]), (where, out["status"], twin["status"])
            _certified(_padded(name, (t, k)), out, kkt.ST_SOLVED, _options("full"), where)
            d = _iteration_differences(out, twin, "defaults", 1, where, failed, WC.ITER_FRAGILE.get((name, kind), ()))
            print(f"[warm] C {where}: worst |iters - iters_twin| {d} (ITER_FRAGILE aside), iterations {int(out['iters'].min())} ... {int(out['iters'].max())}")
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WC.POOLS))
def test_layer_c_as_shipped(name):
    """default options (Anderson columns; a warm-started launch takes no polish): SOLVED, certified, the cold answer"""
    batch = WC.pool(name)
    for kind in WC.FULL_KINDS:
        for fam, (t, k) in _site(name)[1].items():
            where = _where(name, fam, kind, "shipped")
            out = _launch(name, fam, kind, "shipped")
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            assert (out["status"] == 1).all(), (where, out["status"])
            _certified(_padded(name, (t, k)), out, kkt.ST_SOLVED, _options("shipped"), where)
            dx = float(np.abs(out["x"] - H.pad_result(WC.cold_answer(name)["x"], t)).max())
            print(f"[warm] C {where}: |x - x_cold| {dx:.2e} A, iterations {int(out['iters'].min())} ... {int(out['iters'].max())}")
            assert dx <= OC.RATE_TOL, (where, dx)


@pytest.mark.gpu
def test_no_polish_behind_a_warm_start():
    """include/acn_qp.h: a warm-started launch takes no polish.  The stalled pool ends its first pass on a plateau, which is
    what hands a cold launch over to the polish (tests/test_options_gpu.py::test_polish_hand_over_at_an_odd_check_period)"""
    batch = WC.pool("stalled")
    h, shapes = _site("stalled")
    polishing = {fam: s for fam, s in shapes.items() if h.route(*s, batch.B)[1]}
    assert polishing, shapes
    for kind in WC.FULL_KINDS:
        for fam in polishing:
            where = _where("stalled", fam, kind, "shipped")
            before = h.polish_stats()
            out = _launch("stalled", fam, kind, "shipped")
            after = h.polish_stats()
            _written(out, where)
            _dead_periods_zero(batch, out, where)
            assert after["attempted"] == before["attempted"], (where, before, after)
            assert np.isin(out["status"], (1, 2, 5)).all(), (where, out["status"])
            _certified(_padded("stalled", shapes[fam]), out, kkt.ST_SOLVED, _options("shipped"), where)


# ---- D: a retry pass behind a warm pass ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_layer_d_retry_behind_a_warm_pass():
    """stall200_retry1 from ``perturbed`` on the stalled pool: pass 0 starts warm, the retry starts cold -- the twin's
    status and total count, within one check period per pass"""
    batch = WC.pool("stalled")
    _, shapes = _site("stalled")
    assert set(shapes) == {"wave3", "wave4", "long_lds", "tiled_ct1"}, shapes
    failed = []
    for fam, (t, k) in shapes.items():
        where = _where("stalled", fam, "perturbed", "retry")
        out, twin = _launch("stalled", fam, "perturbed", "retry"), WC.twin_padded("stalled", "perturbed", "retry", t)
        _written(out, where)
        _dead_periods_zero(batch, out, where)
        print(f"[warm] D {where}: statuses {np.bincount(out['status'], minlength=6).tolist()}, worst |iters - iters_twin| "
              f"{int(np.abs(out['iters'] - twin['iters']).max())}")
        _status_as_the_twin(out, twin, WC.RETRY_DROPPED, where)
        _certified(_padded("stalled", (t, k)), out, kkt.ST_SOLVED, _options("retry"), where)
        _iteration_differences(out, twin, "stall200_retry1", 2, where, failed)
    assert not failed, failed


# ---- E: stale multipliers at dead periods -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", WC.MIXED)
def test_layer_e_stale_multipliers_at_dead_periods_are_read_as_zero(name):
    """warm_y with U(-3, 3) at every t >= horizon[b] (dead periods inside Tm and the padding): x and y exactly zero there
    after 1, 20 and 60 iterations and as shipped, every output with the bits of the run from ``exact``"""
    batch = WC.pool(name)
    for fam, (t, k) in _site(name)[1].items():
        _, live = WC.masks(batch, t)
        for run in WC.STALE_RUNS + ("shipped",):
            where = _where(name, fam, "stale", run)
            out, ref = _launch(name, fam, "stale", run), _launch(name, fam, "exact", run)
            _written(out, where)
            assert not (out["y"] * ~live).any() and not (out["x"] * ~live).any(), (where, float(np.abs(out["y"] * ~live).max()))
            for key in OUTPUTS:
                assert np.array_equal(out[key], ref[key]), (where, key)
