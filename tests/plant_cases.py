"""The shared cases of the plant tests (tests/test_plant_spec.py, tests/test_plant_gpu.py): a battery table of seven rows
and, for every shape (N, B), a few independent CALLS -- each an input state (s_off, s_len, status), pilots, plug rows and a
plant state (bat, room) -- built so that every branch of the five rules occurs in every shape, N = 1 and B = 1 included:
an element is given one of fifteen situations in rotation, a problem in seven is handed a status that is not accepted,
and a shape with few elements gets more calls.  ``occurrences`` finds the branches again FROM THE DATA, not from the
rotation, and ``check_occurrences`` asserts them: the CPU suite runs it for every shape.

The sites are synthetic: the plant entries read nothing of a site but its number of EVSEs."""
import functools
import math

import numpy as np

from tests import plant_spec as spec

NS, BS = (1, 54, 64, 65, 130), (1, 3, 257)
VOLT, PERIOD = 208.0, 5
K = VOLT * PERIOD / 1e3 / 60          # kWh per ampere-period (aco.py:114)
# (capacity kWh, init_charge kWh, max_power kW, transition_soc) -- None: the "no battery model" row
BATTERIES = ((100.0, 0.0, 7.0, None),      # 0 the reference's test battery: ideal, 33.7 A at 208 V, ample
             (10.0, 9.9, 7.0, None),       # 1 ideal, 0.1 kWh (5.8 A-periods) from full
             (60.0, 0.0, 3.0, None),       # 2 ideal, 14.4 A
             None,                         # 3 no battery model
             (60.0, 30.0, 7.0, 0.8),       # 4 two-stage, plugged in ABOVE the knee (room 30 kWh, knee 12 kWh)
             (60.0, 54.0, 7.0, 0.8),       # 5 two-stage, plugged in BELOW the knee (room 6 kWh)
             (50.0, 25.0, 7.0, 0.5))       # 6 two-stage, plugged in AT the knee: room == knee to the bit
R = len(BATTERIES)
N_SITUATIONS = 15


@functools.lru_cache(maxsize=None)
def table():
    rows = [spec.NO_MODEL if b is None else spec.table_row(*b, VOLT, K) for b in BATTERIES]
    t = np.array(rows, np.float64)
    out = {k: np.ascontiguousarray(t[:, j]) for j, k in enumerate(("t_room", "t_amps", "t_knee", "t_slope"))}
    assert out["t_room"][6] == out["t_knee"][6] > 0
    return out


def _element(kind, rng, t):
    """one EVSE in situation ``kind``: (plug, bat, room, s_off, s_len, pilot)"""
    plug, bat, room, off, ln, pilot = -1, -1, 0.0, 0, int(rng.integers(1, 12)), float(rng.uniform(0.5, 32.0))
    if kind == 0:      # a valid plug replaces whatever was there
        plug, bat, room = int(rng.choice([0, 1, 2, 4, 5, 6])), int(rng.choice([-1, 3])), 7.0
    elif kind == 1:    # keep: an ideal battery with ample room
        bat, room = 0, float(rng.uniform(100.0, 5000.0))
    elif kind == 2:    # a plug beyond the table
        plug, bat = R + int(rng.integers(0, 4)), int(rng.choice([-1, 0]))
        room = 50.0 if bat == 0 else 0.0
    elif kind == 3:    # no slot
        ln, bat, room = 0, 0, 1000.0
    elif kind == 4:    # a slot that has not arrived
        off, bat, room = int(rng.integers(1, 4)), 0, 1000.0
    elif kind == 5:    # no battery
        pass
    elif kind == 6:    # a battery beyond the table
        bat, room = R + int(rng.integers(0, 3)), 12.5
    elif kind == 7:    # the "no battery model" row
        bat, room = 3, math.inf
    elif kind == 8:    # two-stage above the knee
        bat, room = 4, float(t["t_knee"][4] * rng.uniform(1.05, 2.0))
    elif kind == 9:    # two-stage at the knee
        bat, room, pilot = 6, float(t["t_knee"][6]), 32.0
    elif kind == 10:   # two-stage below the knee
        bat, room, pilot = 5, float(t["t_knee"][5] * rng.uniform(0.05, 0.9)), float(rng.uniform(31.0, 32.0))
    elif kind == 11:   # room below the pilot
        bat, room, pilot = 1, float(rng.uniform(0.1, 0.4)), float(rng.uniform(8.0, 32.0))
    elif kind == 12:   # the current limit below the pilot
        bat, room, pilot = 2, 3000.0, float(rng.uniform(20.0, 32.0))
    elif kind == 13:   # nothing offered
        bat, room, pilot = 0, 2000.0, 0.0
    elif kind == 14:   # a negative pilot draws nothing, battery or not
        bat, room, pilot = int(rng.choice([-1, 0])), 2000.0, -1.0
    return plug, bat, room, off, ln, pilot


def n_calls(N, B):
    return max(4 if B == 1 else 2, -(-60 // (B * N)))


@functools.lru_cache(maxsize=None)
def calls(N, B):
    """the calls of shape (N, B): a tuple of dicts cur (s_off, s_len (B, 1, N)), pilots, status, plug, bat, room"""
    rng = np.random.default_rng(1000 * N + B)
    t = table()
    S = n_calls(N, B)
    out = []
    for s in range(S):
        plug, bat, off, ln = (np.empty((B, N), np.int32) for _ in range(4))
        room, pilots = np.empty((B, N)), np.empty((B, N))
        status = np.ones(B, np.int32)
        for b in range(B):
            q = s * B + b
            if q % 7 == 3 or (B == 1 and s == S - 1):
                status[b] = (2, 3, 0, 4)[q % 4]          # MAX_ITER, PRIMAL_INFEASIBLE, UNSET, EMPTY_SET
            elif q % 5 == 1:
                status[b] = spec.SOLVED_INACCURATE
            for i in range(N):
                kind = (q * N + i) % N_SITUATIONS
                if q % 4 == 2 and kind in (2, 6):             # one problem in four holds nothing beyond the table: its flag is 0
                    kind = 5
                plug[b, i], bat[b, i], room[b, i], off[b, i], ln[b, i], pilots[b, i] = _element(kind, rng, t)
        out.append(dict(cur=dict(s_off=off.reshape(B, 1, N), s_len=ln.reshape(B, 1, N)), pilots=pilots, status=status, plug=plug, bat=bat,
                        room=room))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def answers(N, B):
    """tests/plant_spec.py on every call of the shape, computed once"""
    t = table()
    return tuple(spec.plant(c["cur"], c["pilots"], c["status"], t, c["plug"], c["bat"], c["room"]) for c in calls(N, B))


def occurrences(N, B):
    """{branch: how often it occurs over the calls of the shape}, read from the inputs and the specification's answers"""
    t = table()
    count = {}

    def add(name, mask):
        count[name] = count.get(name, 0) + int(np.count_nonzero(mask))

    for c, w in zip(calls(N, B), answers(N, B)):
        off, ln = c["cur"]["s_off"].reshape(B, N), c["cur"]["s_len"].reshape(B, N)
        served = np.isin(c["status"], (spec.SOLVED, spec.SOLVED_INACCURATE))[:, None] & np.ones((B, N), bool)
        present = (ln > 0) & (off == 0)
        offered = present & served & (c["pilots"] > 0)
        plugged = (c["plug"] >= 0) & (c["plug"] < R)
        r = np.where(plugged, c["plug"], c["bat"])                      # the battery the draw reads
        valid = (r >= 0) & (r < R)
        rr = np.where(valid, r, 0)
        room = np.where(plugged, t["t_room"][np.where(plugged, c["plug"], 0)], c["room"])   # the room the draw reads
        knee, amps = t["t_knee"][rr], t["t_amps"][rr]
        add("plug", plugged)
        add("keep", (c["plug"] < 0) & valid)
        add("bad plug", c["plug"] >= R)
        add("absent slot", (ln == 0) & (c["pilots"] > 0))
        add("future slot", (ln > 0) & (off > 0) & (c["pilots"] > 0))
        add("rejected status", ~served & present & (c["pilots"] > 0))
        add("accepted inaccurate", (c["status"] == spec.SOLVED_INACCURATE)[:, None] & offered)
        add("pilot not positive", present & served & (c["pilots"] <= 0))
        add("no battery", offered & (r < 0))
        add("bad battery", offered & (r >= R))
        add("ideal row", offered & valid & (knee == 0) & np.isfinite(amps))
        add("no model row", offered & valid & np.isinf(amps))
        add("above the knee", offered & valid & (knee > 0) & (room > knee))
        add("at the knee", offered & valid & (knee > 0) & (room == knee))
        add("below the knee", offered & valid & (knee > 0) & (room < knee))
        add("room below the pilot", offered & valid & (room < c["pilots"]) & (w["actual"] == room))
        add("current limit below the pilot", offered & valid & (amps < c["pilots"]) & (w["actual"] == amps))
        add("tail below the pilot", offered & valid & (knee > 0) & (w["actual"] < c["pilots"]) & (w["actual"] < amps) & (w["actual"] < room))
        add("flag bad plug", w["flags"] & spec.BAD_PLUG)
        add("flag bad battery", w["flags"] & spec.BAD_BATTERY)
        add("no flag", w["flags"] == 0)
    return count


def check_occurrences(N, B):
    count = occurrences(N, B)
    missing = [k for k, v in count.items() if v == 0]
    assert not missing, (N, B, missing)
    return count


def handle_of(N):
    """a handle of a synthetic site of ``N`` EVSEs behind one row (the plant entries read only N of it)"""
    from adacharge_amd.acn import InfrastructureInfo
    from adacharge_amd.backend import SiteHandle
    from adacharge_amd.builder import make_site

    infra = InfrastructureInfo(np.ones((1, N)), np.array([32.0 * N]), np.zeros(N), np.full(N, VOLT), max_pilot=np.full(N, 32.0),
                               min_pilot=np.full(N, 8.0))
    return SiteHandle(make_site(infra, "LINEAR"), 0)


def plan_of(call):
    from adacharge_amd.backend import PlantPlan

    return PlantPlan(plug=call["plug"], **table())
