"""``simulate_batch(..., session_order=...)``: the closed loop with the two settings that read the session list,
``uninterrupted_charging`` and ``quantize + reallocate``, on the device: advance -> prepare -> solve -> pilots per period.
Six scenarios of caltech54 on the one-wave route (22 steps, Tm = 12): 30 EVs arriving over 10 periods, and a congested
variant of 45 EVs arriving over 6.  Three runs: uninterrupted_charging ("fleet"), quantize + reallocate ("fleet"), all three
(congested, "arrival").  The run with continuous pilots stays on the uncongested fleet, as tests/test_rollout_gpu.py does:
where the site rows bind, a solved schedule meets them to the solver's tolerance, not to ``is_feasible``'s 1e-5 A.
  (a) lockstep, bit for bit at every step: the state the solve read is tests/prepare_spec.py applied to tests/advance_spec.py's
      output of the previous step; the pilots are tests/pilots_spec.py (REALLOCATE with the spec's view, or CONTINUOUS) of
      the device's own schedules
  (b) step 0 equals schedule_batch(postprocess="device", first_period_only=True) with the same settings on the same
      sessions, bit for bit on the scenarios whose spec margins exceed 1e-9 A (at most one of six may fall out)
  (c) invariants over the whole run; the delivered energy against the same loop through schedule_batch and the Python plant
      is printed, not asserted: one level flipped at step 3 is another trajectory, so no tolerance means anything here
Measured figures are printed before they are asserted."""
import functools

import numpy as np
import pytest

from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.postprocessing import _pilot_table
from adacharge_amd.rollout import FleetTable
from tests import advance_spec, helpers, pilots_spec, prepare_cases, prepare_spec

pytestmark = pytest.mark.gpu
B, STEPS, TM = 6, 22, 12
MARGIN = 1e-9
FIXTURES = {"base": dict(n_evs=30, t_span=10), "congested": dict(n_evs=45, t_span=6)}
RUNS = {"uninterrupted": ("base", dict(uninterrupted_charging=True), "fleet"),
        "reallocate": ("base", dict(quantize=True, reallocate=True), "fleet"),
        "all_three": ("congested", dict(uninterrupted_charging=True, quantize=True, reallocate=True), "arrival")}
STATE = ("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap")


def _setup(fixture):
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    rng = np.random.default_rng(77)
    fleets = [helpers.closed_loop_fleet(infra, rng, stay=(8, 13), **FIXTURES[fixture]) for _ in range(B)]
    return infra, iface, fleets


def _alg(iface, **kw):
    alg = AdaptiveSchedulingAlgorithm([ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)], **kw)
    alg.register_interface(iface)
    return alg


@functools.lru_cache(maxsize=None)
def _run(run):
    import torch

    fixture, kw, order = RUNS[run]
    infra, iface, fleets = _setup(fixture)
    alg = _alg(iface, **kw)
    table = FleetTable([[dict(e, max_rate=32.0) for e in f] for f in fleets], infra, iface, alg.objective, STEPS, t_max=TM, session_order=order)
    states = []

    def observer(s, state, pilots):
        torch.cuda.synchronize()
        states.append({k: getattr(state, k).cpu().numpy() for k in STATE + ("x", "status")})

    res = alg.simulate_batch(table, STEPS, return_schedules=True, observer=observer, session_order=order)
    return res, table, states


@functools.lru_cache(maxsize=None)
def _lockstep(run):
    """(a), and what the other tests read: per step the spec's prepare output and the pilots spec's margin"""
    res, table, states = _run(run)
    fixture, kw, order = RUNS[run]
    infra = sites.caltech54()
    site = prepare_cases.site_arrays(infra)
    levels, max_pilot = _pilot_table(infra), np.asarray(infra.max_pilot, float)
    min_rates, realloc = bool(kw.get("uninterrupted_charging")), bool(kw.get("reallocate"))
    keys = table.keys_for("arrival") if min_rates else table.order_keys
    p = table.plan
    plan = {k: getattr(p, k) for k in p._ARRAYS}
    plan.update(done_tol=p.done_tol, kw_per_amp=p.kw_per_amp)
    assert len(states) == STEPS and np.isin(res.status, (1, 5)).all() and not res.flags.any()
    N = infra.num_stations
    seg = (np.arange(B + 1) * N).astype(np.int32)
    prepared, pilot_margin = [], np.full((STEPS, B), np.inf)
    for s in range(STEPS):
        if s == 0:
            prev, applied, status, step = advance_spec.empty_state(B, N, TM, 1), np.zeros((B, N)), None, -1
        else:
            prev, applied, status, step = states[s - 1], res.pilots[s - 1], states[s - 1]["status"], s - 1
        nxt = advance_spec.advance(prev, applied, status, None, None, dict(plan, step=step, a_seg=p.a_seg[s]))
        assert not nxt["flags"].any()
        want = prepare_spec.prepare(nxt, keys[s], site["cre"], site["cim"], site["limits"], site["min_pilot"] if min_rates else None)
        nxt.update(lb=want["lb"], ub=want["ub"])
        for k in STATE:
            assert np.array_equal(states[s][k], nxt[k]), (run, s, k)
        x0 = np.ascontiguousarray(states[s]["x"][:, :, :1])
        if realloc:
            pil, visits, margin = pilots_spec.reallocate(x0, levels, site["cre"], site["cim"], site["limits"], seg, want["v_evse"].ravel(),
                                                         want["v_arrived"].ravel(), want["v_cap"].ravel())
            assert np.array_equal(res.visits[s], visits), (run, s)
            pilot_margin[s] = margin
        else:
            pil = pilots_spec.continuous(x0, max_pilot)
        assert np.array_equal(res.pilots[s], pil[:, :, 0]), (run, s)
        prepared.append(want)
    return prepared, pilot_margin


@pytest.mark.parametrize("run", list(RUNS))
def test_lockstep_with_the_three_specs(run):                                    # (a)
    prepared, _ = _lockstep(run)
    acc = np.stack([w["accepted"] for w in prepared])
    if RUNS[run][1].get("uninterrupted_charging"):
        print(f"[rollout prepare {run}] minimum rates: accepted {(acc == 1).sum()}, refused by the network {(acc == 0).sum()}, "
              f"by the cap {(acc == -1).sum()}")
        assert (acc == 1).any() and ((acc == 0) | (acc == -1)).any()            # some sessions are refused (by the cap: see prepare_cases)
    else:
        assert (acc == -2).all()


def _plant_lists(fleets, t, order):
    lists = [helpers.closed_loop_sessions(f, t) for f in fleets]
    return [sorted(sl, key=lambda x: x.arrival) for sl in lists] if order == "arrival" else lists


@pytest.mark.parametrize("run", list(RUNS))
def test_first_step_equals_schedule_batch(run):                                 # (b)
    res, _, _ = _run(run)
    prepared, pilot_margin = _lockstep(run)
    fixture, kw, order = RUNS[run]
    infra, iface, fleets = _setup(fixture)
    lists = _plant_lists(fleets, 0, order)
    assert sum(len(sl) for sl in lists) > 0
    rates, status = _alg(iface, **kw).schedule_batch(lists, as_arrays=True, postprocess="device", first_period_only=True)
    margin = np.minimum(prepared[0]["margin"], pilot_margin[0])
    keep = margin > MARGIN
    gap = np.abs(rates - res.pilots[0]).max(axis=1)
    print(f"[rollout prepare {run}] step 0: margins (A) {margin.tolist()}; {int((~keep).sum())} of {B} scenarios left out; "
          f"max |pilots - schedule_batch| per scenario = {gap.tolist()}")
    assert (~keep).sum() <= B // 6
    assert np.isin(status, (1, 5)).all() and np.array_equal(rates[keep], res.pilots[0][keep])


@functools.lru_cache(maxsize=None)
def _host_loop(run):
    """the same loop through schedule_batch and the Python plant of tests/helpers.py"""
    fixture, kw, order = RUNS[run]
    infra, iface, fleets = _setup(fixture)
    alg = _alg(iface, **kw)
    for t in range(STEPS):
        iface.data["current_time"] = t
        lists = _plant_lists(fleets, t, order)
        if not any(lists):
            continue
        rates, status = alg.schedule_batch(lists, as_arrays=True, postprocess="device", first_period_only=True)
        for b, f in enumerate(fleets):
            helpers.closed_loop_apply(f, t, rates[b] if status[b] in (1, 5) else np.zeros_like(rates[b]), infra)
    return [np.array([e["delivered"] for e in f]) for f in fleets]


@pytest.mark.parametrize("run", list(RUNS))
def test_closed_loop_invariants(run):                                           # (c)
    res, table, states = _run(run)
    prepared, _ = _lockstep(run)
    fixture, kw, order = RUNS[run]
    infra, iface, fleets = _setup(fixture)
    levels = _pilot_table(infra)
    plugged = np.zeros(res.pilots.shape, dtype=bool)
    print(f"[rollout prepare {run}] worst site-row excess of the applied pilots: "
          f"{max(helpers.infrastructure_violation(res.pilots[:, b].T, infra) for b in range(B)):.3e} A")
    for b, f in enumerate(fleets):
        assert iface.is_feasible({sid: res.pilots[:, b, i] for i, sid in enumerate(infra.station_ids)})
        for e in f:
            plugged[e["arrival"]: e["departure"], b, infra.get_station_index(e["station"])] = True
    assert not res.pilots[~plugged].any()
    assert not res.flags.any() and res.prepare_flags is not None and not res.prepare_flags.any()
    if kw.get("quantize"):
        assert res.pilots.any() and all(np.isin(res.pilots[:, :, i], levels[i]).all() for i in range(infra.num_stations))
    if kw.get("uninterrupted_charging"):
        acc = np.stack([w["accepted"] for w in prepared])
        print(f"[rollout prepare {run}] smallest pilot of an accepted session: {float(res.pilots[acc == 1].min())!r} A")
        assert (res.pilots[acc == 1] >= np.broadcast_to(np.asarray(infra.min_pilot, float), acc.shape)[acc == 1]).all()
        assert not res.pilots[(acc == 0) | (acc == -1)].any()                   # a refused session's first period is pinned to zero
    if kw.get("reallocate"):
        assert res.visits is not None and (res.visits >= 0).all() and res.visits.any()
        x0 = res.x[:, :, :, 0]
        floor = np.stack([pilots_spec.discrete(np.ascontiguousarray(res.x[s][:, :, :1]), levels)[:, :, 0] for s in range(STEPS)])
        agg, low, high = res.pilots.sum(axis=2), floor.sum(axis=2), x0.sum(axis=2) + 1e-7
        print(f"[rollout prepare {run}] reallocation handed back {float((agg - low).sum()):.1f} A-periods of {float((x0.sum(axis=2) - low).sum()):.1f} lost to rounding")
        print(f"[rollout prepare {run}] aggregate - discrete aggregate: min {float((agg - low).min()):.3e} A; aggregate - solved aggregate: max "
              f"{float((agg - x0.sum(axis=2)).max()):.3e} A")
        assert (agg >= low).all() and (agg <= high).all() and (agg > low).any()
    else:
        assert res.visits is None
    host = _host_loop(run)
    requested = sum(e["requested"] for f in fleets for e in f)
    mine, theirs = sum(d.sum() for d in res.delivered), sum(d.sum() for d in host)
    print(f"[rollout prepare {run}] delivered {mine / requested:.6f} of the request on the device, {theirs / requested:.6f} through "
          f"schedule_batch and the Python plant; gap {abs(mine - theirs):.3e} kWh of {requested:.1f} (not asserted)")


def test_the_order_must_be_stated_and_estimate_max_rate_stays_refused():
    infra, iface, fleets = _setup("base")
    for kw, why in ((dict(quantize=True, reallocate=True), "reallocate"), (dict(uninterrupted_charging=True), "uninterrupted_charging")):
        with pytest.raises(ValueError, match=why):
            _alg(iface, **kw).simulate_batch(fleets, 2)
    for order in ("fleet", "arrival"):
        with pytest.raises(ValueError, match="estimate_max_rate"):
            _alg(iface, estimate_max_rate=True).simulate_batch(fleets, 2, session_order=order)
    with pytest.raises(ValueError, match="session_order"):
        _alg(iface).simulate_batch(fleets, 2, session_order="departure")
    table = FleetTable([[dict(e, max_rate=32.0) for e in f] for f in fleets], infra, iface, _alg(iface).objective, 2, session_order="fleet")
    with pytest.raises(ValueError, match="session_order"):
        _alg(iface, quantize=True, reallocate=True).simulate_batch(table, 2, session_order="arrival")
    res = _alg(iface).simulate_batch(table, 2, session_order="fleet")           # an order without a setting that needs it: as before
    plain = _alg(iface).simulate_batch(fleets, 2)
    assert np.array_equal(res.pilots, plain.pilots) and res.visits is None and plain.prepare_flags is None and not res.prepare_flags.any()
