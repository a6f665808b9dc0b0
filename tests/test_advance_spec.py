"""tests/advance_spec.py -- the plain-loop statement of the advance rules (include/acn_qp.h, "time passes") -- reproduces
what the builder builds from the SessionInfo lists of a Python plant, step after step, and answers the unit cases of
tests/advance_cases.py as the rules say.  CPU only: the kernel is held to the same spec in tests/test_advance_gpu.py."""
import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.builder import build_batch_from_table
from adacharge_amd.rollout import FleetTable
from adacharge_amd.session_table import SessionTable
from tests import advance_cases as cases, advance_spec as spec, helpers


def _plan_dict(table, step):
    p = table.plan
    d = {k: getattr(p, k) for k in p._ARRAYS}
    d.update(done_tol=p.done_tol, kw_per_amp=p.kw_per_amp, step=step, a_seg=p.a_seg[step + 1])
    return d


def test_spec_reproduces_the_builder_over_a_closed_loop():
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    evs = helpers.closed_loop_fleet(infra, np.random.default_rng(5))
    steps = 20
    fleet = [dict(station=e["station"], arrival=e["arrival"], departure=e["departure"], requested=e["requested"], max_rate=32.0) for e in evs]
    table = FleetTable([fleet], infra, iface, obj, steps + 1)
    N, Tm = table.N, table.Tm
    k = table.kwh_per_amp_period[0]
    cap0 = max(e["requested"] for e in evs) / k
    state = spec.advance(spec.empty_state(1, N, Tm, 1), np.zeros((1, N)), None, None, None, _plan_dict(table, -1))
    seen = 0
    for t in range(steps):
        assert state["flags"][0] == 0
        sessions = helpers.closed_loop_sessions(evs, t)
        if sessions:
            seen += 1
            want = helpers.pad_batch(build_batch_from_table(SessionTable.from_sessions([sessions], infra), infra, iface, obj), Tm, 1)
            assert state["horizon"][0] == want.T[0]
            for name in ("s_off", "s_len", "lb", "ub", "q", "pdiag", "lf"):
                assert np.array_equal(state[name], getattr(want, name)), (t, name)
            assert state["dc"][0] == want.dc[0] and np.isinf(state["peak"]).all() and want.peak is None
            assert np.abs(state["s_cap"] - want.s_cap).max() <= 8 * (t + 1) * 2.0 ** -52 * max(1.0, cap0), t
        else:
            assert state["horizon"][0] == 1 and not state["s_len"].any() and not state["ub"].any() and not state["lb"].any()
        applied = 0.6 * np.minimum(state["ub"][0, :, 0], state["s_cap"][0, 0])
        served = (state["s_len"][0, 0] > 0) & (state["s_off"][0, 0] == 0)
        after = np.maximum(state["s_cap"][0, 0] - applied, 0.0)[served]
        assert (np.abs(after - table.done_tol) > 1e-6).all()   # no decision of the fixture sits at the done threshold
        helpers.closed_loop_apply(evs, t, applied, infra)
        state = spec.advance(state, applied[None], None, None, None, _plan_dict(table, t))
    assert seen >= 15


def test_spec_with_a_peak_series_and_a_demand_floor():
    """rule 7 reads the series from step + 1, padded with +inf beyond the horizon; rule 8 is one ordered sum"""
    c, applied, status, x, y, plan, _ = cases.make(54, 12, 1)
    out = spec.advance(c, applied, status, x, y, plan)
    for b in range(cases.B):
        hz = out["horizon"][b]
        assert np.array_equal(out["peak"][b, :hz], plan["peak_series"][b, plan["step"] + 1: plan["step"] + 1 + hz])
        assert np.isinf(out["peak"][b, hz:]).all()
        s = 0.0
        for v in applied[b]:
            s = s + (float(v) if status[b] in (1, 5) else 0.0)
        assert out["dfloor"][b] == max(c["dfloor"][b], plan["kw_per_amp"] * s)
    assert out["dfloor"][0] > c["dfloor"][0] and out["dfloor"][2] == c["dfloor"][2] and out["dfloor"][6] == c["dfloor"][6]
    assert np.array_equal(out["warm_x"][:, :, :-1], x[:, :, 1:]) and not out["warm_x"][:, :, -1].any()
    assert np.array_equal(out["warm_y"][:, :, :-1], y[:, :, 1:]) and not out["warm_y"][:, :, -1].any()
    # with a gain the two sessions admitted in problem 0 start at -gain * q' on their windows, nothing else changes
    gained = spec.advance(c, applied, status, x, y, dict(plan, warm_arrival_gain=1e5))
    changed = gained["warm_x"] != out["warm_x"]
    ln = int(out["s_len"][0, 0, 0])
    assert changed[0, :2, :ln].all() and not changed[0, 2:].any() and not changed[0, :2, ln:].any()
    assert np.array_equal(gained["warm_x"][0, :2, :ln], -1e5 * out["q"][0, :2, :ln])
    assert all(np.array_equal(gained[k], out[k]) for k in out if k != "warm_x")


@pytest.mark.parametrize("N,Tm,K", cases.SHAPES)
def test_unit_cases(N, Tm, K):
    c, applied, status, x, y, plan, no_row = cases.make(N, Tm, K)
    out = spec.advance(c, applied, status, x, y, plan)
    top = Tm if Tm < 3 else Tm - 1
    ln, off, cap = out["s_len"], out["s_off"], out["s_cap"]
    # every live window lies inside the horizon, bounds are zero outside the live windows of arrived-or-kept sessions
    for b in range(cases.B):
        live = np.zeros((N, Tm), bool)
        for k in range(K):
            for i in range(N):
                if ln[b, k, i] > 0:
                    assert 0 <= off[b, k, i] and off[b, k, i] + ln[b, k, i] <= out["horizon"][b] <= Tm
                    live[i, off[b, k, i]: off[b, k, i] + ln[b, k, i]] = True
                else:
                    assert off[b, k, i] == 0 and cap[b, k, i] == 0.0
        if b != 5:   # (problem 5 carries bounds of slots that were never valid)
            assert not out["ub"][b][~live].any() and not out["lb"][b][~live].any()
        assert (out["ub"][b] >= out["lb"][b]).all()
    # problem 0: both arrivals admitted, the second with max < min -> ub = lb
    alen = max(1, min(top - 1, 5))
    assert out["flags"][0] == 0 and ln[0, 0, 0] == alen and ln[0, K - 1, 1] == alen
    assert (out["lb"][0, 1, :alen] == 6.0).all() and (out["ub"][0, 1, :alen] == 6.0).all()
    # problem 1: retired by length, by cap (exactly, below the tolerance, clamped), one survivor
    assert not ln[1, 0, [0, 1, 2, 4]].any() and not out["ub"][1, [0, 1, 2, 4]].any()
    if top > 1:
        assert ln[1, 0, 3] == top - 1 and cap[1, 0, 3] == 20.0 - 3.0 and (out["lb"][1, 3, : top - 1] == 1.0).all()
        assert out["horizon"][1] == top - 1
    # problem 2: the future session moves one period closer, nothing is taken from its cap
    if Tm >= 2 and top > 1:
        assert (off[2, K - 1, 0], ln[2, K - 1, 0], cap[2, K - 1, 0]) == (0, top - 1, 64.0)
        assert (out["ub"][2, 0, : top - 1] == 16.0).all()
    if top >= 3 and K > 1:
        assert (off[2, 0, 1], ln[2, 0, 1]) == (0, 1) and (off[2, 1, 1], ln[2, 1, 1]) == (1, top - 2)
        assert ln[2, 0, 2] == 1 and out["flags"][2] == 0
    # problem 4: idle
    assert out["horizon"][4] == 1 and not ln[4].any() and not out["ub"][4].any() and out["flags"][4] == 0
    # problem 5: every refusal reason raises bit 1 and changes nothing; the bad slots raise bit 4; one arrival is admitted
    assert out["flags"][5] == spec.REFUSED | spec.BAD_SLOT | (spec.NO_ROW if no_row is not None else 0)
    assert ln[5, 0, 1] == 1 and not ln[5, 0, 2:4].any()
    if K > 1:
        assert ln[5, 1, 0] == 0
    if no_row is not None:
        assert out["horizon"][5] == no_row and not out["q"][5].any() and out["pdiag"][5] == 0.0 and out["lf"][5] == 0.0
        assert all(out["flags"][b] & spec.NO_ROW == 0 and np.array_equal(out["q"][b], plan["q_table"][plan["h_row"][out["horizon"][b]]])
                   for b in range(cases.B) if b != 5)
    # each refusal reason on its own
    seg = plan["a_seg"]
    recs = range(seg[5], seg[6])
    admitted = 0
    for r in recs:
        p1 = dict(plan)
        p1["a_seg"] = np.r_[np.zeros(6, np.int32), 0, 0].astype(np.int32)
        p1["a_seg"][5:7] = r, r + 1
        p1["a_seg"][6:] = r + 1
        p1["a_seg"][:5] = r
        one = spec.advance_one(5, c, applied, status, None, None, p1)
        admitted += 0 if one["flags"] & spec.REFUSED else 1
    # the record on EVSE 1 and its twin are each fine alone; every other record is refused alone too (with Tm = 1 the window
    # on EVSE 0 ends in this step, so the record behind it is fine as well)
    assert admitted == (3 if Tm == 1 else 2)
    # problem 6: nothing delivered
    served = (c["s_len"][6] > 0) & (c["s_off"][6] == 0) & (c["s_len"][6] > 1) & (c["s_cap"][6] > cases.DONE_TOL)
    assert served.any() or Tm == 1
    assert np.array_equal(cap[6][served], c["s_cap"][6][served]) and out["dfloor"][6] == c["dfloor"][6]
    # Tm = 1: whatever was there is over
    if Tm == 1:
        assert (out["horizon"] == 1).all() and ln.sum() == 4   # only the admitted arrivals: two of problem 0, two of problem 5


def test_missing_row_everywhere():
    c, applied, status, x, y, plan, _ = cases.make(5, 1, 1)
    plan = dict(plan, h_row=np.full(2, -1, np.int32))
    out = spec.advance(c, applied, status, x, y, plan)
    assert (out["flags"] & spec.NO_ROW).all() and not out["q"].any() and not out["pdiag"].any()
