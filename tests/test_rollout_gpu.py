"""``AdaptiveSchedulingAlgorithm.simulate_batch``: a closed loop of solve -> pilots -> advance with the state resident in
HBM.  Six scenarios of caltech54 on the one-wave route (stays of 8-12 periods, 22 steps) and on the two-wave route (stays
up to 24 periods, 34 steps):
  (a) lockstep: every downloaded state equals tests/advance_spec.py applied to the previous one and its pilots, bit for bit
  (b) step 0's pilots equal schedule_batch(postprocess="device", first_period_only=True) on the same sessions, bit for bit
  (c) the invariants of test_closed_loop_mpc_delivers_all_energy, the delivered energy against the same loop through
      schedule_batch and a Python plant (margin: 1e-4 * 32 A per plugged EVSE-period, summed)
  (d) idle scenarios (every EV departed) come back SOLVED with x = 0
  (e) warm_start=True: same pilots within the parity tolerance, no more iterations in total (one-wave route)
  (f) quantize=True: the pilots are tests/pilots_spec.py DISCRETE of the device's own schedules, bit for bit
Measured figures are printed before they are asserted."""
import functools

import numpy as np
import pytest

from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.rollout import FleetTable
from tests import advance_spec as spec, helpers, pilots_spec

pytestmark = pytest.mark.gpu
PARITY = 1e-4 * 32.0     # the project's parity tolerance, amperes
ROUTES = {"one_wave": dict(stay=(8, 13), steps=22, t_max=12, route="wave1"), "two_wave": dict(stay=(13, 25), steps=34, t_max=24, route="wave2")}
B, N_EVS = 6, 30
STATE = ("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap")


def _setup(route):
    cfg = ROUTES[route]
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    rng = np.random.default_rng(77)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=N_EVS, t_span=10, stay=cfg["stay"]) for _ in range(B)]
    return cfg, infra, iface, fleets


def _alg(iface, **kw):
    alg = AdaptiveSchedulingAlgorithm([ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)], **kw)
    alg.register_interface(iface)
    return alg


@functools.lru_cache(maxsize=None)
def _run(route, warm=False, quantize=False, watch=False):
    import torch

    cfg, infra, iface, fleets = _setup(route)
    alg = _alg(iface, quantize=quantize)
    table = FleetTable([[dict(e, max_rate=32.0) for e in f] for f in fleets], infra, iface, alg.objective, cfg["steps"], t_max=cfg["t_max"])
    states = []

    def observer(s, state, pilots):
        torch.cuda.synchronize()
        states.append({k: getattr(state, k).cpu().numpy() for k in STATE + ("x", "status")})

    res = alg.simulate_batch(table, cfg["steps"], warm_start=warm, return_schedules=True, observer=observer if watch else None)
    return res, table, states


@functools.lru_cache(maxsize=None)
def _host_loop(route):
    """the same loop through schedule_batch and the Python plant of tests/helpers.py"""
    cfg, infra, iface, fleets = _setup(route)
    alg = _alg(iface)
    applied = np.zeros((cfg["steps"], B, infra.num_stations))
    for t in range(cfg["steps"]):
        iface.data["current_time"] = t
        lists = [helpers.closed_loop_sessions(f, t) for f in fleets]
        if not any(lists):
            continue
        rates, status = alg.schedule_batch(lists, as_arrays=True, postprocess="device", first_period_only=True)
        assert np.isin(status, (1, 5)).all()
        applied[t] = rates
        for b, f in enumerate(fleets):
            helpers.closed_loop_apply(f, t, rates[b], infra)
    return applied, [np.array([e["delivered"] for e in f]) for f in fleets]


@pytest.mark.parametrize("route", list(ROUTES))
def test_lockstep_with_the_spec_and_idle_scenarios(route):
    res, table, states = _run(route, watch=True)
    cfg = ROUTES[route]
    from adacharge_amd.adaptive_charging_optimization import _site_handle

    assert _site_handle(sites.caltech54(), "SOC", False, 0)[1].route(cfg["t_max"], 1, B)[0] == cfg["route"]
    assert len(states) == cfg["steps"] and not res.flags.any()
    p = table.plan
    plan = {k: getattr(p, k) for k in p._ARRAYS}
    plan.update(done_tol=p.done_tol, kw_per_amp=p.kw_per_amp)
    raw = res.pilots
    idle = 0
    for s in range(cfg["steps"]):
        st = states[s]
        assert np.isin(st["status"], (1, 5)).all(), (s, st["status"])
        if s + 1 < cfg["steps"]:                                              # (a)
            want = spec.advance(st, raw[s], st["status"], None, None, dict(plan, step=s, a_seg=p.a_seg[s + 1]))
            for k in STATE:
                assert np.array_equal(states[s + 1][k], want[k]), (s, k)
            assert not want["flags"].any()
        for b in range(B):                                                    # (d)
            if not st["s_len"][b].any():
                idle += 1
                assert st["horizon"][b] == 1 and st["status"][b] == 1 and not st["x"][b].any() and not raw[s, b].any()
    assert idle >= B   # the last step at least: every EV has departed
    assert np.array_equal(res.x, np.stack([st["x"] for st in states]))


@pytest.mark.parametrize("route", list(ROUTES))
def test_first_step_equals_schedule_batch(route):                             # (b)
    res, _, _ = _run(route, watch=True)
    cfg, infra, iface, fleets = _setup(route)
    lists = [helpers.closed_loop_sessions(f, 0) for f in fleets]
    assert sum(len(sl) for sl in lists) > 0
    rates, status = _alg(iface).schedule_batch(lists, as_arrays=True, postprocess="device", first_period_only=True)
    gap = float(np.abs(rates - res.pilots[0]).max())
    print(f"[rollout {route}] step 0: max |pilots - schedule_batch| = {gap:.3e} A (bit equal: {np.array_equal(rates, res.pilots[0])})")
    assert np.isin(status, (1, 5)).all() and np.array_equal(rates, res.pilots[0])   # measured: 0 A on both routes


@pytest.mark.parametrize("route", list(ROUTES))
def test_closed_loop_invariants_and_delivered_energy(route):                  # (c)
    res, table, _ = _run(route, watch=True)
    cfg, infra, iface, fleets = _setup(route)
    plugged = np.zeros(res.pilots.shape, dtype=bool)
    for b, f in enumerate(fleets):
        assert iface.is_feasible({sid: res.pilots[:, b, i] for i, sid in enumerate(infra.station_ids)})
        for e in f:
            plugged[e["arrival"]: e["departure"], b, infra.get_station_index(e["station"])] = True
    assert not res.pilots[~plugged].any() and not res.flags.any()
    host_applied, host_delivered = _host_loop(route)
    k = table.kwh_per_amp_period[0]
    requested = sum(e["requested"] for f in fleets for e in f)
    mine, theirs = sum(d.sum() for d in res.delivered), sum(d.sum() for d in host_delivered)
    margin = PARITY * k * int(plugged[: cfg["steps"]].sum())
    print(f"[rollout {route}] delivered {mine / requested:.6f} of the request on the device, {theirs / requested:.6f} through "
          f"schedule_batch; gap {abs(mine - theirs):.3e} kWh (margin {margin:.3e}); worst pilot gap {np.abs(host_applied - res.pilots).max():.3e} A")
    assert abs(mine - theirs) <= margin


def test_warm_start_same_pilots_fewer_iterations():                           # (e)
    """Measured on an MI355X: max |pilots warm - cold| = 4.6e-05 A; 3,260 iterations warm against 3,300 cold (2,640 of either are
    the floor of 20 iterations per solve, the first residual check).  The sessions admitted in a step start where a cold
    solve starts them (``acnqp_advance_plan.warm_arrival_gain``): with zeros there the warm run took 7,020 iterations."""
    cold, _, _ = _run("one_wave", watch=True)
    warm, _, _ = _run("one_wave", warm=True)
    gap = float(np.abs(warm.pilots - cold.pilots).max())
    print(f"[rollout warm] max |pilots warm - cold| = {gap:.3e} A; iterations warm {int(warm.iters.sum())}, cold {int(cold.iters.sum())}")
    print(f"[rollout warm] per step, warm: {warm.iters.sum(axis=1).tolist()}")
    print(f"[rollout warm] per step, cold: {cold.iters.sum(axis=1).tolist()}")
    assert np.isin(warm.status, (1, 5)).all() and not warm.flags.any()
    assert gap <= PARITY
    assert warm.iters.sum() <= cold.iters.sum()


def test_quantized_pilots_are_the_spec_of_the_device_schedules():             # (f)
    from adacharge_amd.postprocessing import _pilot_table

    res, _, _ = _run("one_wave", quantize=True)
    levels = _pilot_table(sites.caltech54())
    assert np.isin(res.status, (1, 5)).all() and not res.flags.any()
    for s in range(res.pilots.shape[0]):
        assert np.array_equal(res.pilots[s], pilots_spec.discrete(res.x[s][:, :, :1], levels)[:, :, 0]), s
    assert res.pilots.any() and np.isin(res.pilots, levels[0]).all()


def test_settings_the_rollout_refuses():
    cfg, infra, iface, fleets = _setup("one_wave")
    for kw, why in ((dict(quantize=True, reallocate=True), "reallocate"), (dict(estimate_max_rate=True), "estimate_max_rate"),
                    (dict(uninterrupted_charging=True), "uninterrupted_charging")):
        with pytest.raises(ValueError, match=why):
            _alg(iface, **kw).simulate_batch(fleets, 2)
