"""The shared pools of the prepare tests (tests/test_prepare_spec.py, tests/test_prepare_gpu.py).  A pool is a slot state
(s_off, s_len, s_cap (B, 1, N)), bounds (lb, ub (B, N, Tm)), keys (B, N) and a site in the SOC form of ``acnqp_pilot_plan``
(cre, cim (M, N), limits (M,), min_pilot (N,)).

Two kinds:
  * ``fleet_pool``: snapshots of ``helpers.closed_loop_fleet`` at a few clock values, with the SessionInfo lists they come
    from -- what ties tests/prepare_spec.py to ``session_table.apply_minimum_charging_rate`` and ``pilot_plan_arrays``
  * ``random_pool``: random slot states of any shape (N, Tm), for the kernel's paths: one wavefront and four, bounds that
    need reconciling, equal keys, a slot that has not arrived

caltech54's rows cannot refuse a minimum pilot: with all 54 EVSEs at 8 A its worst row carries 208 A against 416.7 A, and
a pod of eight carries at most 24 A against 80 A.  The "caltech54" pools therefore use the site DERATED to a quarter of its
limits (pods of 20 A: three EVSEs of one phase pair at 8 A are refused), so that the 54-EVSE shape sees refusals by the
network; the rollout test runs on the site as it is."""
import numpy as np

from adacharge_amd import ObjectiveComponent, quick_charge, sites
from adacharge_amd.acn import Interface

DERATE = 0.25
FIVE_FRACTION = 0.3   # limits of the 5-EVSE site: pod 9.6 A, phase pairs 19.2, 19.2, 9.6 A, primaries 6.35, 8.31, 6.35 A


def site_of(name):
    if name == "caltech54":
        infra = sites.caltech54()
        infra.constraint_limits = np.asarray(infra.constraint_limits, float) * DERATE
        return infra
    if name == "five":
        return sites.balanced_three_phase(5, pods=1, load_fraction=FIVE_FRACTION, name="FV")
    if name.startswith("balanced"):
        return sites.balanced_three_phase(int(name[8:]), pods=4, load_fraction=0.2, name="BL")
    return getattr(sites, name)()


def site_arrays(infra):
    cm = np.asarray(infra.constraint_matrix, float)
    ph = np.deg2rad(infra.phases)
    return dict(cre=np.ascontiguousarray(cm * np.cos(ph)), cim=np.ascontiguousarray(cm * np.sin(ph)),
                limits=np.ascontiguousarray(infra.constraint_limits, float), min_pilot=np.ascontiguousarray(infra.min_pilot, float))


def fleet_pool(name, seed, n_snap=16, clocks=(3, 6, 9, 12)):
    """``n_snap`` snapshots of one site: a fresh ``closed_loop_fleet`` each, looked at at one of ``clocks``, every plugged EV
    part-charged (one in six within 0.13 kWh -- under one period at 8 A and 208 V -- of its request).  Returns a dict:
    infra, iface, lists (SessionInfo lists in fleet order), fleets, clocks."""
    from tests import helpers

    infra = site_of(name)
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(seed)
    n_evs = min(45, infra.num_stations)
    lists, fleets, ts = [], [], []
    for k in range(n_snap):
        t = clocks[k % len(clocks)]
        fleet = helpers.closed_loop_fleet(infra, rng, n_evs=n_evs, t_span=12)
        for e in fleet:
            if e["arrival"] <= t:
                left = rng.uniform(0.01, 0.13) if rng.random() < 1 / 6 else e["requested"] * rng.uniform(0.2, 1.0)
                e["delivered"] = max(0.0, e["requested"] - left)
        lists.append(helpers.closed_loop_sessions(fleet, t))
        fleets.append(fleet)
        ts.append(t)
    return dict(infra=infra, iface=iface, lists=lists, fleets=fleets, clocks=ts, objective=[ObjectiveComponent(quick_charge)])


def keys_of(lists, infra, order):
    """(B, N) int32: the position of every session in its list ("fleet"), or its rank by (arrival, position) ("arrival")"""
    key = np.zeros((len(lists), infra.num_stations), np.int32)
    for b, sl in enumerate(lists):
        pos = list(range(len(sl))) if order == "fleet" else np.argsort(np.argsort([s.arrival for s in sl], kind="stable"), kind="stable")
        for k, s in enumerate(sl):
            key[b, infra.get_station_index(s.station_id)] = pos[k]
    return key


def random_pool(name, Tm, B=7, seed=0):
    """Random slot states of the site ``name`` at horizon ``Tm``: dict(cur, key, site).  Problem 5 carries a live slot that
    has not arrived (flag 1); keys repeat; some caps lie under the minimum pilot; some bounds need reconciling."""
    infra = site_of(name)
    N = infra.num_stations
    rng = np.random.default_rng(seed + 1000 * N + Tm)
    s_len = np.where(rng.random((B, 1, N)) < 0.75, rng.integers(1, Tm + 1, size=(B, 1, N)), 0).astype(np.int32)
    s_off = np.zeros((B, 1, N), np.int32)
    s_cap = np.where(rng.random((B, 1, N)) < 0.2, rng.uniform(0.5, 7.9, size=(B, 1, N)), rng.uniform(8.0, 200.0, size=(B, 1, N)))
    if Tm > 1:
        i = int(np.flatnonzero(s_len[5, 0] > 0)[0])
        s_off[5, 0, i], s_len[5, 0, i] = 1, Tm - 1
    lb, ub = np.zeros((B, N, Tm)), np.zeros((B, N, Tm))
    for b in range(B):
        for i in range(N):
            n, o = int(s_len[b, 0, i]), int(s_off[b, 0, i])
            lb[b, i, o:o + n] = rng.choice([0.0, 0.0, 0.0, 6.0, 12.0], size=n)
            ub[b, i, o:o + n] = np.maximum(lb[b, i, o:o + n], rng.choice([32.0, 32.0, 16.0, 7.0], size=n))
    key = rng.integers(0, max(2, N // 2), size=(B, N)).astype(np.int32)   # (equal keys: the EVSE index decides)
    return dict(cur=dict(lb=lb, ub=ub, s_off=s_off, s_len=s_len, s_cap=np.where(s_len > 0, s_cap, 0.0)), key=key, site=site_arrays(infra),
                infra=infra)


SHAPES = (("caltech54", 12), ("five", 3), ("balanced64", 2), ("balanced65", 2), ("wide128", 4))


def subset(pool, b):
    """problem ``b`` of a random pool alone"""
    cur = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in pool["cur"].items()}
    return dict(cur=cur, key=np.ascontiguousarray(pool["key"][b:b + 1]), site=pool["site"], infra=pool["infra"])


def handle_of(infra):
    from adacharge_amd.backend import SiteHandle
    from adacharge_amd.builder import make_site

    return SiteHandle(make_site(infra, "SOC"), 0)


def plan_of(pool):
    from adacharge_amd.backend import PreparePlan

    return PreparePlan(key=pool["key"], **pool["site"])


if __name__ == "__main__":   # the host entry on one random pool, for a test that sets ACNQP_POST_CHUNK for a whole process
    import sys

    pool = random_pool(sys.argv[1], int(sys.argv[2]))
    h = handle_of(pool["infra"])
    np.savez(sys.argv[3], **h.prepare_host(pool["cur"], plan_of(pool)))
    h.close()
