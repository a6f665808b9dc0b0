"""tests/advance_priced_spec.py -- the advance rules with a clock cost (rule 6b of include/acn_qp.h) -- is the plain spec
without a cost, and with one reproduces what the builder builds from the SessionInfo lists of a Python plant under a
time-of-use tariff, step after step, with the interface's clock moved: q bit for bit.  ``rollout.FleetTable`` splits
``tou_energy_cost`` out of the objective and still refuses what it cannot carry.  CPU only: the kernel is held to the same
spec in tests/test_advance_priced_gpu.py."""
import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites, total_energy, tou_energy_cost
from adacharge_amd.acn import Interface
from adacharge_amd.adaptive_charging_optimization import QuadObjective
from adacharge_amd.builder import build_batch_from_table
from adacharge_amd.rollout import FleetTable
from adacharge_amd.session_table import SessionTable
from tests import advance_cases as cases, advance_priced_spec as priced, advance_spec as spec, helpers

R = 0.15   # $/kWh: what a delivered kWh is worth (total_energy's coefficient)


@pytest.mark.parametrize("N,Tm,K", cases.SHAPES)
def test_without_a_cost_it_is_the_plain_spec(N, Tm, K):                      # (i)
    made = cases.make(N, Tm, K)
    want, got = spec.advance(*made[:6]), priced.advance(*made[:6], cost=None)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_spec_reproduces_the_priced_builder_over_a_closed_loop():             # (ii)
    infra = sites.caltech54()
    steps = 20
    evs = helpers.closed_loop_fleet(infra, np.random.default_rng(5))
    fleet = [dict(station=e["station"], arrival=e["arrival"], departure=e["departure"], requested=e["requested"], max_rate=32.0) for e in evs]
    longest = max(e["departure"] - e["arrival"] for e in evs)
    prices = 0.05 + 0.2 * np.random.default_rng(11).random(steps + 1 + longest)
    assert len(set(prices.tolist())) == len(prices) and (prices > R).sum() >= 5 and (prices < R).sum() >= 5
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0, "prices": prices})
    obj = [ObjectiveComponent(total_energy, R), ObjectiveComponent(equal_share, 1e-12), ObjectiveComponent(tou_energy_cost)]
    table = FleetTable([fleet], infra, iface, obj, steps + 1)
    assert iface.data["current_time"] == 0 and table.plan.c_coef == 1.0 and table.plan.c_series.shape == (1, steps + 1 + table.Tm)
    N, Tm = table.N, table.Tm
    k = table.kwh_per_amp_period[0]
    cap0 = max(e["requested"] for e in evs) / k
    state = priced.advance(spec.empty_state(1, N, Tm, 1), np.zeros((1, N)), None, None, None, *priced.plan_and_cost(table, -1))
    seen = 0
    for t in range(steps):
        assert state["flags"][0] == 0
        iface.data["current_time"] = t
        sessions = helpers.closed_loop_sessions(evs, t)
        if sessions:
            seen += 1
            want = helpers.pad_batch(build_batch_from_table(SessionTable.from_sessions([sessions], infra), infra, iface, obj), Tm, 1)
            assert state["horizon"][0] == want.T[0]
            for name in ("s_off", "s_len", "lb", "ub", "q", "pdiag", "lf"):
                assert np.array_equal(state[name], getattr(want, name)), (t, name)
            hz = int(state["horizon"][0])
            assert state["q"][0, :, :hz].all() and not state["q"][0, :, hz:].any()      # priced inside the horizon, padding beyond
            assert np.abs(state["s_cap"] - want.s_cap).max() <= 8 * (t + 1) * 2.0 ** -52 * max(1.0, cap0), t
        else:
            assert state["horizon"][0] == 1 and not state["s_len"].any() and not state["ub"].any() and not state["lb"].any()
        applied = 0.6 * np.minimum(state["ub"][0, :, 0], state["s_cap"][0, 0])
        helpers.closed_loop_apply(evs, t, applied, infra)
        state = priced.advance(state, applied[None], None, None, None, *priced.plan_and_cost(table, t))
    assert seen >= 12


def test_rule_6b_and_rule_9_on_the_unit_cases():
    """q' is the table's row plus coef * (weight * price) inside the new horizon and the row itself beyond; a problem without
    a row keeps q' = 0; a session admitted in the step starts at -gain * that q'"""
    c, applied, status, x, y, plan, no_row = cases.make(54, 12, 1)
    rng = np.random.default_rng(3)
    cost = dict(coef=-1.75, weight=rng.uniform(0.01, 0.03, 54), series=rng.uniform(0.05, 0.4, (cases.B, plan["step"] + 1 + 12)))
    plain = spec.advance(c, applied, status, x, y, plan)
    out = priced.advance(c, applied, status, x, y, plan, cost)
    for k in plain:
        assert k == "q" or np.array_equal(out[k], plain[k]), k
    for b in range(cases.B):
        hz = out["horizon"][b]
        if b == 5:
            assert no_row is not None and not out["q"][b].any()
            continue
        add = cost["coef"] * (cost["weight"][:, None] * cost["series"][b, plan["step"] + 1: plan["step"] + 1 + hz][None, :])
        assert np.array_equal(out["q"][b, :, :hz], plain["q"][b, :, :hz] + add) and np.array_equal(out["q"][b, :, hz:], plain["q"][b, :, hz:])
    gained = priced.advance(c, applied, status, x, y, dict(plan, warm_arrival_gain=1e5), cost)
    ln = int(out["s_len"][0, 0, 0])
    assert np.array_equal(gained["warm_x"][0, :2, :ln], -1e5 * out["q"][0, :2, :ln])
    changed = gained["warm_x"] != out["warm_x"]
    assert changed[0, :2, :ln].all() and not changed[0, 2:].any() and not changed[0, :2, ln:].any()
    assert all(np.array_equal(gained[k], out[k]) for k in out if k != "warm_x")


# ---- FleetTable (iii) -------------------------------------------------------------------------------------------------------
def _table(obj, prices_len=40, steps=6, B=2, **kw):
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0, "prices": 0.1 + 0.01 * np.arange(prices_len)})
    rng = np.random.default_rng(2)
    fleets = [[dict(e, max_rate=32.0) for e in helpers.closed_loop_fleet(infra, rng, n_evs=5, t_span=3, stay=(3, 6))] for _ in range(B)]
    return FleetTable(fleets, infra, iface, obj, steps, **kw)


def test_fleet_table_refusals_and_prices():
    tou = ObjectiveComponent(tou_energy_cost)
    base = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    with pytest.raises(ValueError, match="2 tou_energy_cost components"):
        _table(base + [tou, ObjectiveComponent(tou_energy_cost, 2.0)])
    ok = _table(base + [tou, ObjectiveComponent(tou_energy_cost, 0)])             # a zero coefficient prices nothing
    assert ok.plan.c_coef == 1.0 and ok.plan.c_series.shape == (2, 6 + ok.Tm)
    assert np.array_equal(ok.plan.c_series[1], 0.1 + 0.01 * np.arange(6 + ok.Tm))
    assert np.array_equal(ok.plan.c_weight, np.asarray(sites.caltech54().voltages, float) / 1e3 * (5 / 60))
    assert np.array_equal(ok.plan.q_table, _table(base).plan.q_table)              # the other components build the table as before
    with pytest.raises(ValueError, match=f"needs steps \\+ t_max = {6 + ok.Tm}"):
        _table(base + [tou], prices_len=6 + ok.Tm - 1)

    def clock_reader(rates, infrastructure, interface, **kwargs):
        return QuadObjective(np.full(rates.shape, float(interface.current_time)))

    with pytest.raises(ValueError, match="depends on the clock"):
        _table(base + [tou, ObjectiveComponent(clock_reader)])
    with pytest.raises(ValueError, match="depends on the clock"):
        _table(base + [ObjectiveComponent(clock_reader)])
    assert _table(base).plan.c_series is None and _table(base).plan.c_coef is None
    with pytest.raises(ValueError, match="no tou_energy_cost"):
        _table(base, prices=np.ones(40))
    # prices=: one tariff per scenario, entry 0 at start_time, in place of the interface's
    P = 6 + ok.Tm
    two = np.stack([0.2 + 0.001 * np.arange(P + 3), 0.4 - 0.002 * np.arange(P + 3)])
    t = _table(base + [ObjectiveComponent(tou_energy_cost, 3.0)], prices=two, start_time=1)
    assert t.plan.c_coef == 3.0 and np.array_equal(t.plan.c_series, two[:, :P])
    assert np.array_equal(_table(base + [tou], prices=two[1]).plan.c_series, np.stack([two[1, :P]] * 2))
    with pytest.raises(ValueError, match="needs steps"):
        _table(base + [tou], prices=two[:, : P - 1])
    with pytest.raises(ValueError, match="shape"):
        _table(base + [tou], prices=np.ones((3, P)))
