"""``simulate_batch(resolve="events")``: a scenario is solved afresh only at step 0, where an EV of its fleet plugs in or
unplugs, and every ``max_recompute`` periods; in between it plays the schedule it holds.  The six fleets of the mask test
(tests/test_hold_spec.py): five EVs each on caltech54, 26 steps at Tm = 12, every record with max_rate = 32 A, a peak limit
of 40 A so that a site row binds, quick_charge + equal_share * 1e-12.
  (a) max_recompute = 1: pilots, status, iters, flags and x of the default call, bit for bit; solved is all true
  (b) max_recompute None and 4: solved is ``resolve_rows``, held steps made no iteration, and every array of the result is
      that of a TWIN, bit for bit, statuses included.  The twin is written here from the SiteHandle entries the loop had
      before, with torch ``index_select`` and indexed assignment where the loop runs the select and hold kernels: its solves
      have the same launch sizes
  (c) invariants of those runs: no pilot where no EV is plugged, feasible per scenario, no EV delivered more than it
      asked for, every status accepted, no flag
  (d) with warm_start, with a two-stage battery per scenario, and with tou_energy_cost last in the list under a (B, P)
      tariff: max_recompute None against the twin, bit for bit
  (e) estimate_max_rate, uninterrupted_charging and an unknown ``resolve`` are refused with the reason"""
import functools

import numpy as np
import pytest

from adacharge_amd import (AdaptiveSchedulingAlgorithm, ObjectiveComponent, SimpleRampdown, equal_share, quick_charge, sites,
                           tou_energy_cost)
from adacharge_amd.acn import Interface
from adacharge_amd.rollout import FleetTable
from tests import helpers

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_library")]
B, N_EVS, STEPS, TM, PEAK = 6, 5, 26, 12, 40.0
PARITY = 1e-4 * 32.0     # the project's parity tolerance, amperes (tests/test_rollout_gpu.py)
ARRAYS = ("pilots", "status", "iters", "flags", "x", "actual", "plant_flags", "energy_cost")


def _setup(kind="plain"):
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    rng = np.random.default_rng(77)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=N_EVS, t_span=14, stay=(8, 13)) for _ in range(B)]
    fleets = [[dict(e, max_rate=32.0) for e in f] for f in fleets]
    if kind == "battery":   # one EV per scenario plugs in past its transition_soc: it draws less than it is offered
        for f in fleets:
            cap = 2.0 * f[0]["requested"] / 0.15
            f[0] = dict(f[0], battery=dict(capacity=cap, init_charge=0.85 * cap, max_power=7.0, transition_soc=0.8))
    return infra, iface, fleets


def _alg(iface, kind="plain", **kw):
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    if kind == "tou":
        obj.append(ObjectiveComponent(tou_energy_cost, 0.5))
    alg = AdaptiveSchedulingAlgorithm(obj, peak_limit=PEAK, **kw)
    alg.register_interface(iface)
    return alg


def _table(kind, infra, iface, fleets, alg):
    prices = None
    if kind == "tou":
        prices = np.random.default_rng(5).uniform(0.05, 0.4, (B, STEPS + TM))
    return FleetTable(fleets, infra, iface, alg.objective, STEPS, t_max=TM, peak_limit=PEAK, prices=prices)


@functools.lru_cache(maxsize=None)
def _run(kind="plain", resolve="events", max_recompute=None, warm=False):
    infra, iface, fleets = _setup(kind)
    alg = _alg(iface, kind, max_recompute=max_recompute)
    table = _table(kind, infra, iface, fleets, alg)
    return alg.simulate_batch(table, STEPS, warm_start=warm, return_schedules=True, resolve=resolve), table


@functools.lru_cache(maxsize=None)
def _twin(kind="plain", max_recompute=None, warm=False):
    """the events loop from the entries the every-step loop is made of; torch gathers and scatters in place of the two kernels"""
    import torch
    from adacharge_amd import backend
    from adacharge_amd.adaptive_charging_optimization import _site_handle
    from adacharge_amd.backend import DeviceBatch
    from adacharge_amd.postprocessing import pilot_plan_arrays
    from adacharge_amd.rollout import START_GAIN

    infra, iface, fleets = _setup(kind)
    alg = _alg(iface, kind, max_recompute=max_recompute)
    table = _table(kind, infra, iface, fleets, alg)
    mask = table.resolve_rows(max_recompute)
    site, handle = _site_handle(infra, alg.constraint_type, table.has_peak, alg.device, with_flat=table.need_flat, with_max=table.need_max)
    options = backend.default_options()
    dev = torch.device("cuda", handle.device)
    N, K = table.N, table.K
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        plan = table.plan.to_device(dev)
        plan.warm_arrival_gain = START_GAIN if warm else 0.0
        pplan = pilot_plan_arrays(None, infra, iface, "continuous", batch=B, t_max=TM).to_device(dev)
        want_y = warm and site.Mg > 0
        bufs = [DeviceBatch.empty(site, B, TM, K, dev, want_y=want_y, dfloor=table.dfloor0) for _ in range(2)]
        new = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        pilots, xs = new(STEPS, B, N), new(STEPS, B, N, TM)
        status, iters, flags = (new(STEPS, B, dt=torch.int32) for _ in range(3))
        wx, wy = new(B, N, TM), new(B, site.Mg, TM) if want_y else None
        actual = plflags = None
        if table.has_plant:
            plplan = table.plant_plan.to_device(dev)
            bat, room = torch.full((B, N), -1, dtype=torch.int32, device=dev), new(B, N)
            actual, plflags = new(STEPS, B, N), new(STEPS, B, dt=torch.int32)
        handle.advance_device(bufs[1], bufs[0], new(B, N), plan, -1, flags[0], use_status=False, stream=stream, seg_row=0)
        for s in range(STEPS):
            cur, nxt = bufs[s % 2], bufs[(s + 1) % 2]
            warm_now = want_y and s > 0
            rows = np.flatnonzero(mask[s])
            if len(rows) == B:
                handle.solve_device(cur, options, stream=stream, warm_x=wx if warm_now else None, warm_y=wy if warm_now else None)
            else:
                held = torch.where(wx > cur.ub, cur.ub, wx)                  # rule H2: two comparisons, in this order
                held = torch.where(held < cur.lb, cur.lb, held)
                cur.x.copy_(held)
                cur.status.copy_(status[s - 1])
                cur.iters.zero_()
                if want_y:
                    cur.y.copy_(wy)
                if len(rows):
                    idx = torch.from_numpy(rows).to(dev)
                    dense = DeviceBatch.empty(site, len(rows), TM, K, dev, want_y=want_y)
                    for k in backend._PROBLEM_ARRAYS:
                        setattr(dense, k, getattr(cur, k).index_select(0, idx))
                    handle.solve_device(dense, options, stream=stream, warm_x=wx.index_select(0, idx) if warm_now else None,
                                        warm_y=wy.index_select(0, idx) if warm_now else None)
                    cur.x[idx], cur.status[idx], cur.iters[idx] = dense.x, dense.status, dense.iters
                    if want_y:
                        cur.y[idx] = dense.y
            handle.pilots_device(pplan, cur.x, first=pilots[s], stream=stream)
            if actual is not None:
                handle.plant_device(cur, plplan, pilots[s], bat, room, actual[s], plflags[s], status=cur.status, plug_row=s, stream=stream)
            status[s].copy_(cur.status)
            iters[s].copy_(cur.iters)
            xs[s].copy_(cur.x)
            if s + 1 < STEPS:
                handle.advance_device(cur, nxt, pilots[s] if actual is None else actual[s], plan, s, flags[s + 1], use_status=True, warm_x=wx,
                                      warm_y=wy, stream=stream, seg_row=s + 1)
        torch.cuda.synchronize(dev)
    p, st = pilots.cpu().numpy(), status.cpu().numpy()
    p[~np.isin(st, backend.ACCEPTED_STATUSES)] = 0.0
    drawn = p if actual is None else actual.cpu().numpy()
    return dict(pilots=p, status=st, iters=iters.cpu().numpy(), flags=flags.cpu().numpy(), x=xs.cpu().numpy(),
                actual=None if actual is None else drawn, plant_flags=None if plflags is None else plflags.cpu().numpy(),
                energy_cost=table.energy_cost(drawn), delivered=table.delivered(drawn))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _equals_twin(res, twin):
    for k in ARRAYS:
        a, b = getattr(res, k), twin[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
    assert all(np.array_equal(a, b) for a, b in zip(res.delivered, twin["delivered"]))


def test_max_recompute_one_is_the_default_run():                              # (a)
    every, _ = _run(resolve="every_step")
    res, table = _run(max_recompute=1)
    assert every.solved is None and every.resolve_flags is None
    assert res.solved.shape == (STEPS, B) and res.solved.dtype == bool and res.solved.all() and not res.resolve_flags.any()
    for k in ("pilots", "status", "iters", "flags", "x"):
        assert np.array_equal(_bits(getattr(res, k)), _bits(getattr(every, k))), k
    assert res.pilots.any() and np.isin(every.status, (1, 5)).all()
    # "every_step" ignores max_recompute, as before
    other, _ = _run(resolve="every_step", max_recompute=4)
    assert np.array_equal(_bits(other.pilots), _bits(every.pilots)) and other.solved is None


@pytest.mark.parametrize("max_recompute", [None, 4])
def test_events_equal_the_twin_bit_for_bit(max_recompute):                    # (b)
    res, table = _run(max_recompute=max_recompute)
    mask = table.resolve_rows(max_recompute)
    assert np.array_equal(res.solved, mask) and not mask.all() and (mask.sum(axis=1) == 0).any() and (mask.sum(axis=1) == 1).any()
    assert not res.iters[~res.solved].any() and (res.iters[res.solved] > 0).any()
    _equals_twin(res, _twin(max_recompute=max_recompute))
    every, _ = _run(resolve="every_step")
    print(f"[rollout events] max_recompute={max_recompute}: {int(mask.sum())} of {mask.size} (step, scenario) pairs solved; iterations "
          f"{int(res.iters.sum())} against {int(every.iters.sum())} every step; worst pilot gap to the every-step run "
          f"{np.abs(res.pilots - every.pilots).max():.3e} A")
    assert np.array_equal(res.pilots[0], every.pilots[0])                     # step 0 is everyone's


@pytest.mark.parametrize("max_recompute", [None, 4])
def test_invariants_of_a_held_run(max_recompute):                             # (c)
    res, table = _run(max_recompute=max_recompute)
    infra, iface, fleets = _setup()
    assert np.isin(res.status, (1, 5)).all() and not res.flags.any() and not res.resolve_flags.any()
    plugged = np.zeros(res.pilots.shape, dtype=bool)
    k = table.kwh_per_amp_period[0]
    for b, f in enumerate(fleets):
        assert iface.is_feasible({sid: res.pilots[:, b, i] for i, sid in enumerate(infra.station_ids)})
        for n, e in enumerate(f):
            i = infra.get_station_index(e["station"])
            plugged[e["arrival"]: e["departure"], b, i] = True
            got = float(res.pilots[e["arrival"]: e["departure"], b, i].sum()) * k
            # the request to the parity tolerance per period of the stay (the solver meets an energy row to its tolerance)
            assert got <= e["requested"] + PARITY * k * (e["departure"] - e["arrival"]), (b, n)
            assert res.delivered[b][n] <= e["requested"]
    assert not res.pilots[~plugged].any() and res.pilots[plugged].any() and (res.pilots >= 0).all()
    assert (res.pilots.sum(axis=2) <= PEAK + PARITY).all() and (res.pilots.sum(axis=2) >= PEAK - PARITY).any()   # the peak row binds


@pytest.mark.parametrize("kind,warm", [("plain", True), ("battery", False), ("tou", False)])
def test_events_with_warm_start_batteries_and_a_tariff(kind, warm):           # (d)
    res, table = _run(kind, warm=warm)
    assert np.array_equal(res.solved, table.resolve_rows(None)) and not res.iters[~res.solved].any()
    assert np.isin(res.status, (1, 5)).all() and not res.flags.any() and not res.resolve_flags.any()
    assert (res.actual is not None) == (kind == "battery") and (res.energy_cost is not None) == (kind == "tou")
    if kind == "battery":
        assert (res.actual < res.pilots).any() and not res.plant_flags.any()   # a held schedule does not see what the battery drew
    _equals_twin(res, _twin(kind, warm=warm))


def test_what_a_held_schedule_cannot_serve_is_refused():                      # (e)
    infra, iface, fleets = _setup()
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]

    def call(resolve="events", **kw):
        alg = AdaptiveSchedulingAlgorithm(obj, peak_limit=PEAK, **kw)
        alg.register_interface(iface)
        order = "fleet" if kw.get("uninterrupted_charging") else None
        table = FleetTable(fleets, infra, iface, obj, STEPS, t_max=TM, peak_limit=PEAK, session_order=order)
        return alg.simulate_batch(table, STEPS, session_order=order, resolve=resolve)

    with pytest.raises(ValueError, match="estimate_max_rate: the reference's estimator runs inside schedule"):
        call(estimate_max_rate=True, max_rate_estimator=SimpleRampdown())
    with pytest.raises(ValueError, match="uninterrupted_charging: its minimum-rate step is per solve"):
        call(uninterrupted_charging=True)
    with pytest.raises(ValueError, match='resolve must be "every_step" or "events", not \'sometimes\''):
        call(resolve="sometimes")
