"""tests/plant_spec.py -- the yardstick of the plant kernel -- against what a battery must do, on the CPU:
  * bounds: 0 <= actual <= min(offer, current limit, room) and room' == room - actual >= 0, exactly
  * an EVSE without a battery and the "no battery model" row draw the offer, bit for bit
  * the two-stage tail: at the knee its rate does not exceed the current limit, past it the draw does not grow as room shrinks
  * the battery of the reference's acnsim integration tests (100 kWh, empty, 7 kW): 32 A passes at 208 V, 240 V caps it
  * fill: chained with tests/advance_spec.py over 30 periods, no battery is overfilled and what was drawn is the room used
  * every branch of the rules occurs in every shape of tests/plant_cases.py (what the GPU test runs)
  * ``rollout.FleetTable``: the table and the plug rows of a hand-made fleet, a fleet without batteries builds the advance
    plan it built before the plant existed (tests/golden/plant_parent_plan.npz, written by tools/make_golden_plant_plan.py
    on the commit before), every bad battery field is refused
  * the two flag constants of include/acn_qp.h, compiled by gcc, are the binding's"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, backend, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.rollout import FleetTable
from tests import advance_spec, plant_cases as cases, plant_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _random_states(seed, n=4000):
    rng = np.random.default_rng(seed)
    t = cases.table()
    for _ in range(n):
        r = int(rng.integers(-1, cases.R))
        room = math.inf if r == 3 else float(rng.choice([0.0, rng.uniform(0, 40), rng.uniform(0, 6000)]))
        plug = int(rng.choice([-1, -1, rng.integers(0, cases.R)]))
        yield t, plug, r, room, float(rng.choice([0.0, -2.0, rng.uniform(0, 40)])), bool(rng.random() < 0.9)


def test_bounds_hold_exactly_on_random_states():
    seen = 0
    for t, plug, r, room, pilot, served in _random_states(1):
        nb, nroom, a, f = spec.plant_one(cases.R, t["t_room"], t["t_amps"], t["t_knee"], t["t_slope"], plug, r, room, 0, 3, pilot, served)
        assert f == 0
        p = pilot if served and pilot > 0 else 0.0
        before = t["t_room"][plug] if plug >= 0 else room
        assert nb == (plug if plug >= 0 else r)
        if nb < 0:
            assert a == p and nroom == before
            continue
        assert 0.0 <= a <= min(p, t["t_amps"][nb], before)
        assert nroom == before - a and nroom >= 0.0
        seen += a < p
    assert seen > 500   # the battery binds often enough for the bounds to mean something


def test_no_battery_and_the_no_model_row_draw_the_offer_bit_for_bit():
    t = cases.table()
    rng = np.random.default_rng(2)
    for _ in range(500):
        pilot = float(rng.uniform(0, 1e4))
        for bat, room, plug in ((-1, 0.0, -1), (-1, 123.0, -1), (3, math.inf, -1), (0, 5.0, 3), (-7, 1.0, -3)):
            nb, nroom, a, f = spec.plant_one(cases.R, t["t_room"], t["t_amps"], t["t_knee"], t["t_slope"], plug, bat, room, 0, 1, pilot, True)
            assert a == pilot and f == 0 and nb == (3 if plug == 3 else bat)
            assert nroom == (math.inf if nb == 3 else room)


def test_the_tail_meets_the_current_limit_at_the_knee_and_falls_with_the_room():
    t = cases.table()
    for r in (4, 5, 6):
        knee, amps, slope = t["t_knee"][r], t["t_amps"][r], t["t_slope"][r]
        at = spec.plant_one(cases.R, t["t_room"], t["t_amps"], t["t_knee"], t["t_slope"], -1, r, knee, 0, 1, 1e3, True)[2]
        assert at <= amps and at >= amps * (1 - 4e-16)       # one division on the host, one product here: two roundings
        above = spec.plant_one(cases.R, t["t_room"], t["t_amps"], t["t_knee"], t["t_slope"], -1, r, knee * 1.5, 0, 1, 1e3, True)[2]
        assert above == amps
        last = at
        for frac in np.linspace(1.0, 0.0, 200):
            a = spec.plant_one(cases.R, t["t_room"], t["t_amps"], t["t_knee"], t["t_slope"], -1, r, knee * frac, 0, 1, 1e3, True)[2]
            assert a <= last and a == min(knee * frac * slope, amps, knee * frac)
            last = a
        assert last == 0.0


def test_the_reference_battery_passes_32_amps_at_208_volts_and_caps_at_240():
    """acnsim.Battery(100, 0, 7) of the reference's integration tests"""
    for volt, want in ((208.0, 32.0), (240.0, 7000 / 240)):
        assert (7000 / 208 > 32) and (7000 / 240 < 32)
        row = spec.table_row(100.0, 0.0, 7.0, None, volt, volt * 5 / 1e3 / 60)
        cols = [[v] for v in row]
        nb, room, a, f = spec.plant_one(1, *cols, 0, -1, 0.0, 0, 4, 32.0, True)
        assert a == want and nb == 0 and f == 0 and room == row[0] - want and row[2] == row[3] == 0.0


def test_fill_no_battery_is_overfilled_and_the_draw_is_the_room_used():
    B, N, Tm, steps = 2, cases.R, 31, 30
    t = cases.table()
    cur = advance_spec.empty_state(B, N, Tm, 1)
    cur["s_len"][:] = Tm
    cur["s_cap"][:] = 1e6
    cur["ub"][:] = 32.0
    plan = dict(q_table=np.zeros((Tm, N, Tm)), h_scal=np.zeros((Tm, 3)), h_row=np.r_[-1, np.arange(Tm)].astype(np.int32), done_tol=1e-9,
                kw_per_amp=0.208, a_seg=None)
    pilots = np.stack([np.full(N, 32.0), np.linspace(3.0, 31.0, N)])
    bat, room = np.full((B, N), -1, np.int32), np.zeros((B, N))
    plug0 = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    drawn, cap0 = np.zeros((B, N)), cur["s_cap"][:, 0].copy()
    for s in range(steps):
        out = spec.plant(cur, pilots, None, t, plug0 if s == 0 else np.full((B, N), -1, np.int32), bat, room)
        assert not out["flags"].any() and (out["room"] >= 0).all() and (out["actual"] >= 0).all() and (out["actual"] <= pilots).all()
        bat, room = out["bat"], out["room"]
        drawn += out["actual"]
        cur = advance_spec.advance(cur, out["actual"], None, None, None, dict(plan, step=s))
    model = np.isfinite(t["t_room"])
    used = t["t_room"][None, model] - room[:, model]
    assert np.abs(drawn[:, model] - used).max() <= 2 * steps * np.finfo(float).eps * t["t_room"][model].max()   # 30 subtractions and 30 additions
    assert (room[:, 1] == 0.0).all() and (drawn[:, 1] > 0).all()           # the battery 0.1 kWh from full is full
    assert (drawn[:, ~model] == steps * pilots[:, ~model]).all()
    assert (cur["s_len"] == Tm - steps).all() and np.abs(cur["s_cap"][:, 0] - (cap0 - drawn)).max() <= 1e-6   # the advance took what was drawn


@pytest.mark.parametrize("N", cases.NS)
@pytest.mark.parametrize("B", cases.BS)
def test_every_branch_occurs_in_every_shape(N, B):
    count = cases.check_occurrences(N, B)
    assert len(count) == 21


# ---- rollout.FleetTable ----------------------------------------------------------------------------------------------
def _site():
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    return infra, iface, [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]


def test_fleet_table_builds_the_battery_table_and_the_plug_rows():
    infra, iface, obj = _site()
    ids = infra.station_ids
    k, volt = 208.0 * 5 / 1e3 / 60, 208.0
    assert np.all(np.asarray(infra.voltages) == volt)
    two = dict(capacity=60.0, init_charge=54.0, max_power=6.6, transition_soc=0.8)
    ideal = dict(capacity=100.0, init_charge=0.0, max_power=7.0)
    fleets = [[dict(station=ids[3], arrival=0, departure=5, requested=4.0, max_rate=32.0, battery=two),
               dict(station=ids[7], arrival=2, departure=6, requested=3.0, max_rate=32.0),
               dict(station=ids[9], arrival=40, departure=44, requested=3.0, max_rate=32.0, battery=ideal),     # beyond the run: not admitted
               dict(station=ids[3], arrival=5, departure=8, requested=2.0, max_rate=32.0, battery=dict(ideal, transition_soc=None))],
              [dict(station=ids[0], arrival=-2, departure=4, requested=5.0, max_rate=32.0, battery=ideal)]]
    table = FleetTable(fleets, infra, iface, obj, steps=8, t_max=6)
    assert table.has_plant
    p = table.plant_plan
    rows = [spec.table_row(60.0, 54.0, 6.6, 0.8, volt, k), spec.NO_MODEL, spec.table_row(100.0, 0.0, 7.0, None, volt, k),
            spec.table_row(100.0, 0.0, 7.0, None, volt, k)]
    for j, name in enumerate(("t_room", "t_amps", "t_knee", "t_slope")):
        assert np.array_equal(getattr(p, name), np.array([r[j] for r in rows])), name
    assert p.t_knee[0] == (1 - 0.8) * 60.0 / k and p.t_slope[0] == p.t_amps[0] / p.t_knee[0] and p.t_room[0] == (60.0 - 54.0) / k
    want = np.full((8, 2, 54), -1, np.int32)
    want[0, 0, 3], want[2, 0, 7], want[5, 0, 3], want[0, 1, 0] = 0, 1, 2, 3
    assert p.plug.dtype == np.int32 and np.array_equal(p.plug, want)
    # the same EVs without batteries: the same advance plan, no plant
    bare = FleetTable([[{k2: v for k2, v in e.items() if k2 != "battery"} for e in f] for f in fleets], infra, iface, obj, steps=8, t_max=6)
    assert not bare.has_plant and bare.plant_plan is None
    for name in backend.AdvancePlan._ARRAYS:
        a, b = getattr(table.plan, name), getattr(bare.plan, name)
        assert (a is None and b is None) or np.array_equal(a, b), name


def test_a_fleet_without_batteries_builds_the_plan_of_the_commit_before():
    import make_golden_plant_plan as golden

    want = np.load(os.path.join(ROOT, "tests", "golden", "plant_parent_plan.npz"))
    table = golden.table()
    assert not table.has_plant and table.plant_plan is None
    got = golden.arrays(table)
    assert sorted(got) == sorted(want.files) and len(got) >= 12
    for name in want.files:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("field,value,match", [
    ("capacity", 0.0, "capacity"), ("capacity", -1.0, "capacity"), ("capacity", float("nan"), "capacity"), ("capacity", float("inf"), "capacity"),
    ("init_charge", -0.1, "init_charge"), ("init_charge", 60.5, "init_charge"), ("init_charge", float("nan"), "init_charge"),
    ("max_power", 0.0, "max_power"), ("max_power", -7.0, "max_power"), ("max_power", float("inf"), "max_power"),
    ("transition_soc", 0.0, "transition_soc"), ("transition_soc", 1.0, "transition_soc"), ("transition_soc", 1.5, "transition_soc"),
    ("transition_soc", float("nan"), "transition_soc"), ("capacity", None, "needs numbers"), ("max_power", "fast", "needs numbers")])
def test_every_bad_battery_field_is_refused(field, value, match):
    infra, iface, obj = _site()
    good = dict(capacity=60.0, init_charge=30.0, max_power=7.0, transition_soc=0.8)
    ev = dict(station=infra.station_ids[1], sid="ev-x", arrival=0, departure=5, requested=4.0, max_rate=32.0)
    assert FleetTable([[ev], [dict(ev, battery=good)]], infra, iface, obj, steps=4).has_plant
    with pytest.raises(ValueError, match=rf"scenario 1, EV 0 \(ev-x\): battery.*{match}"):
        FleetTable([[ev], [dict(ev, battery=dict(good, **{field: value}))]], infra, iface, obj, steps=4)
    missing = {k: v for k, v in good.items() if k != "init_charge"}
    with pytest.raises(ValueError, match="scenario 0, EV 0.*needs numbers"):
        FleetTable([[dict(ev, battery=missing)]], infra, iface, obj, steps=4)
    # a battery of an EV the run never admits is validated all the same
    with pytest.raises(ValueError, match="scenario 0, EV 1"):
        FleetTable([[ev, dict(ev, arrival=90, departure=95, battery=dict(good, capacity=-1.0))]], infra, iface, obj, steps=4)


# ---- the constants, by the method of tests/test_abi.py -----------------------------------------------------------------
def test_the_plant_constants_match_the_header(tmp_path):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acn_qp.h")).read(), flags=re.S)
    consts = re.findall(r"#define\s+(ACNQP_PLANT_\w+)\b", text)
    assert sorted(consts) == ["ACNQP_PLANT_BAD_BATTERY", "ACNQP_PLANT_BAD_PLUG"]
    src, exe = tmp_path / "plant.c", tmp_path / "plant"
    src.write_text('#include <stdio.h>\n#include "acn_qp.h"\nint main(void) {\n' + "\n".join(f'printf("%d\\n", {c});' for c in consts)
                   + "\nreturn 0;\n}\n")
    cc = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    value = {c[len("ACNQP_"):]: int(v) for c, v in zip(consts, got)}
    assert value == {k: getattr(backend, k) for k in value} == dict(PLANT_BAD_PLUG=spec.BAD_PLUG, PLANT_BAD_BATTERY=spec.BAD_BATTERY)
    assert {"acnqp_plant_device", "acnqp_plant_host"} <= set(backend.EXPORTED_SYMBOLS)
    assert re.search(r"int\s+acnqp_plant_device\s*\(", text) and re.search(r"int\s+acnqp_plant_host\s*\(", text)
