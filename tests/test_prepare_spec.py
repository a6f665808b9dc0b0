"""tests/prepare_spec.py (the yardstick of the prepare kernel) against the host path it stands for, without a GPU:
  * rule 2 equals ``session_table.apply_minimum_charging_rate -> build_batch_from_table`` in period 0 of lb and ub
  * rule 3 equals ``pilot_plan_arrays(..., "reallocate")`` of that table: visiting order, s_arrived, s_cap
on snapshots of ``helpers.closed_loop_fleet`` (tests/prepare_cases.py), wherever the spec's margin exceeds 1e-9 A -- the
host path sums with BLAS and compares a hypot, the spec sums in increasing i and compares squares.
s_cap is compared to 16 ulp where it is the remaining demand: the slot state holds ``kWh / (V * period / 1e3 / 60)``
(aco.py:114, two roundings in the divisor and one division), ``pilot_plan_arrays`` holds ``kWh * 1000 / V * 60 / period``
(four roundings) -- seven roundings of 2^-53 between them, 16 ulp with room; where the cap is a rate bound it is compared
exactly.
And ``rollout.FleetTable.order_keys``: the list positions of ``helpers.closed_loop_sessions`` at every step."""
import functools

import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, quick_charge, session_table as st, sites
from adacharge_amd.acn import Interface
from adacharge_amd.builder import build_batch_from_table
from adacharge_amd.postprocessing import pilot_plan_arrays
from tests import helpers, prepare_cases as cases, prepare_spec as spec

MARGIN = 1e-9          # amperes
SEEDS = {"caltech54": 11, "jpl52": 12, "five": 13}


@functools.lru_cache(maxsize=None)
def _pool(name):
    pool = cases.fleet_pool(name, SEEDS[name])
    infra, iface = pool["infra"], pool["iface"]
    table = st.enforce_pilot_limit(st.SessionTable.from_sessions(pool["lists"], infra), infra)       # ada.py:141
    batch = build_batch_from_table(table, infra, iface, pool["objective"])
    assert batch.K == 1
    cur = dict(lb=batch.lb, ub=batch.ub, s_off=batch.s_off, s_len=batch.s_len, s_cap=batch.s_cap)
    return pool, table, batch, cur


def _same_cap(got, want):
    return got == want or abs(got - want) <= 16 * np.spacing(abs(want))


@pytest.mark.parametrize("name", list(SEEDS))
def test_rule_2_is_the_minimum_rate_step_and_rule_3_the_pilot_plan(name):
    pool, table, batch, cur = _pool(name)
    infra, iface = pool["infra"], pool["iface"]
    site = cases.site_arrays(infra)
    key = cases.keys_of(pool["lists"], infra, "arrival")
    got = spec.prepare(cur, key, **site)
    raised = st.apply_minimum_charging_rate(table, infra, iface.period)                             # ada.py:147-150
    want = build_batch_from_table(raised, infra, iface, pool["objective"])
    plan = pilot_plan_arrays(raised, infra, iface, "reallocate")
    B = batch.B
    under = [b for b in range(B) if not got["margin"][b] > MARGIN]
    print(f"[prepare spec {name}] margins (A): min {got['margin'].min():.3e}; {len(under)} of {B} snapshots under {MARGIN:g}")
    assert len(under) <= B // 16          # (the seeds above: none)
    acc = got["accepted"]
    print(f"[prepare spec {name}] accepted {(acc == 1).sum()}, refused by the network {(acc == 0).sum()}, by the cap {(acc == -1).sum()}")
    assert (acc == 1).any() and (acc == 0).any() and (acc == -1).any()
    ties = 0
    for b in range(B):
        arr = [s.arrival for s in pool["lists"][b]]
        ties += len(arr) - len(set(arr))
        if b in under:
            continue
        assert np.array_equal(got["lb"][b, :, 0], want.lb[b, :, 0]) and np.array_equal(got["ub"][b, :, 0], want.ub[b, :, 0]), b
        assert np.array_equal(got["lb"][b, :, 1:], batch.lb[b, :, 1:]) and np.array_equal(got["ub"][b, :, 1:], batch.ub[b, :, 1:]), b
        lo, hi = int(plan.sess_seg[b]), int(plan.sess_seg[b + 1])
        n = hi - lo
        assert n == int((batch.s_len[b] > 0).sum())
        assert np.array_equal(got["v_evse"][b, :n], plan.s_evse[lo:hi]) and np.array_equal(got["v_arrived"][b, :n], plan.s_arrived[lo:hi]), b
        assert not got["v_arrived"][b, n:].any() and not got["v_cap"][b, n:].any()
        assert sorted(got["v_evse"][b].tolist()) == list(range(infra.num_stations))
        for r in range(n):
            i = int(got["v_evse"][b, r])
            g, w = float(got["v_cap"][b, r]), float(plan.s_cap[lo + r])
            assert (g == w) if g == got["ub"][b, i, 0] and w == g else _same_cap(g, w), (b, r, g, w)
    assert ties > 0        # equal arrivals: the list position decides
    assert not got["flags"].any()


@pytest.mark.parametrize("name", list(SEEDS))
def test_view_in_fleet_order_without_minimum_rates(name):
    pool, table, batch, cur = _pool(name)
    infra, iface = pool["infra"], pool["iface"]
    got = spec.prepare(cur, cases.keys_of(pool["lists"], infra, "fleet"), None, None, None, None)
    plan = pilot_plan_arrays(table, infra, iface, "reallocate")
    assert np.array_equal(got["lb"], batch.lb) and np.array_equal(got["ub"], batch.ub) and np.isinf(got["margin"]).all()
    for b in range(batch.B):
        lo, hi = int(plan.sess_seg[b]), int(plan.sess_seg[b + 1])
        n = hi - lo
        assert np.array_equal(got["v_evse"][b, :n], plan.s_evse[lo:hi]) and np.array_equal(got["v_arrived"][b, :n], plan.s_arrived[lo:hi])
        assert all(_same_cap(float(g), float(w)) for g, w in zip(got["v_cap"][b, :n], plan.s_cap[lo:hi]))


def test_five_evses_by_hand():
    """balanced_three_phase(5, pods=1) at 0.3 of full load: EVSEs 0, 1 on AB (+30 deg), 2, 3 on BC (-90 deg), 4 on CA (+150 deg);
    the pod row over all five carries 9.6 A.  At 8 A each, in the order 0 .. 4: EVSE 0 alone puts 8 A on the pod (accepted);
    0 and 1 put 16 A (refused); 0 and 2 put |8 /30 + 8 /-90| = 8 A (accepted); 0, 2 and 3 put |8 /30 + 16 /-90| = 13.9 A
    (refused); 0, 2 and 4 are balanced: 0 A on the pod, 8 A on CA's 9.6 A (accepted).  In the order 1, 0, 3, 2, 4 the roles
    of each pair swap.  The other rows (pairs 19.2, 19.2 A; primaries 6.35, 8.31, 6.35 A against at most 3.46 A) never bind."""
    infra = cases.site_of("five")
    site = cases.site_arrays(infra)
    N, Tm = 5, 3
    cur = dict(lb=np.zeros((1, N, Tm)), ub=np.full((1, N, Tm), 32.0), s_off=np.zeros((1, 1, N), np.int32), s_len=np.full((1, 1, N), Tm, np.int32),
               s_cap=np.full((1, 1, N), 50.0))
    for key, acc in (([0, 1, 2, 3, 4], [1, 0, 1, 0, 1]), ([1, 0, 3, 2, 4], [0, 1, 0, 1, 1]), ([0, 0, 0, 0, 0], [1, 0, 1, 0, 1])):
        got = spec.prepare(cur, np.array([key], np.int32), **site)
        assert got["accepted"][0].tolist() == acc
        assert got["lb"][0, :, 0].tolist() == [8.0 * a for a in acc] and got["ub"][0, :, 0].tolist() == [32.0 * a for a in acc]
        assert got["v_evse"][0].tolist() == sorted(range(N), key=lambda i: (key[i], i))
        assert got["v_cap"][0].tolist() == [32.0 * acc[i] for i in got["v_evse"][0]] and got["v_arrived"][0].all()
        assert got["margin"][0] > 1.0
    # a cap under the minimum pilot refuses whatever the network says; a bound above it stays; a bound under it is raised
    cur["s_cap"][0, 0, 0] = 7.5
    cur["lb"][0, 2, 0], cur["ub"][0, 4, 0] = 12.0, 6.0
    got = spec.prepare(cur, np.array([[0, 1, 2, 3, 4]], np.int32), **site)
    assert got["accepted"][0].tolist() == [-1, 1, 1, 0, 1]      # (EVSE 1 takes the place EVSE 0 had)
    assert got["lb"][0, :, 0].tolist() == [0.0, 8.0, 12.0, 0.0, 8.0] and got["ub"][0, :, 0].tolist() == [0.0, 32.0, 32.0, 0.0, 8.0]
    assert got["v_cap"][0].tolist() == [0.0, 32.0, 32.0, 0.0, 8.0]


def test_fleet_table_order_keys():
    """``order_keys[s, b, i]`` orders the EVSEs exactly as the plant's list of step s does, for both stated orders"""
    from adacharge_amd.rollout import FleetTable

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    rng = np.random.default_rng(5)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=30, t_span=10, stay=(8, 13)) for _ in range(3)]
    steps, start = 22, 2                      # (start 2: some EVs arrived before the run; "arrival" ranks their true arrival)
    obj = [ObjectiveComponent(quick_charge)]
    args = ([[dict(e, max_rate=32.0) for e in f] for f in fleets], infra, iface, obj, steps, start)
    assert FleetTable(*args).order_keys is None and FleetTable(*args, session_order=None).session_order is None
    with pytest.raises(ValueError, match="session_order"):
        FleetTable(*args, session_order="departure")
    seen_tie = False
    for order in ("fleet", "arrival"):
        table = FleetTable(*args, session_order=order)
        keys = table.order_keys
        assert keys.shape == (steps, 3, infra.num_stations) and keys.dtype == np.int32
        assert np.array_equal(table.min_pilot, np.asarray(infra.min_pilot, float))
        for s in range(steps):
            for b, f in enumerate(fleets):
                sl = helpers.closed_loop_sessions(f, start + s)
                if order == "arrival":
                    seen_tie |= len({x.arrival for x in sl}) < len(sl)
                    sl = sorted(sl, key=lambda x: x.arrival)                  # stable: plug-in order, the list position decides ties
                evses = [infra.get_station_index(x.station_id) for x in sl]
                ks = [int(keys[s, b, i]) for i in evses]
                assert ks == sorted(ks) and len(set(ks)) == len(ks), (order, s, b)
    assert seen_tie
