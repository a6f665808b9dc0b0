"""Shared test helpers: golden-fixture loading and the four invariants the
reference's own test base class asserts (t_aco.py:50-83)."""
import os

import numpy as np

from adacharge_amd import sites
from adacharge_amd.acn import Interface, SessionInfo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caltech54_T12.npz")


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_case(g, key):
    """Rebuild the SessionInfo list of fixture ``key``; returns
    (sessions, meta dict, expected dict)."""
    st = g[f"{key}_station"]
    sessions = []
    for k in range(len(st)):
        rem = int(g[f"{key}_departure"][k] - g[f"{key}_arrival"][k])
        mins = np.zeros(rem)
        mins[0] = g[f"{key}_min0"][k]
        sessions.append(
            SessionInfo(
                str(st[k]), f"s{k}", float(g[f"{key}_demand"][k]), 0.0,
                int(g[f"{key}_arrival"][k]), int(g[f"{key}_departure"][k]),
                current_time=0, min_rates=mins, max_rates=float(g[f"{key}_maxr"][k]),
            )
        )
    m = g[f"{key}_meta"]
    meta = dict(seed=int(m[0]), ct="SOC" if m[1] else "LINEAR", es=float(m[2]), eq=bool(m[3]), T=int(m[4]))
    exp = {k: g[f"{key}_{k}"] for k in ("rates", "obj", "agg") if f"{key}_{k}" in g}
    return sessions, meta, exp


def caltech_interface():
    infra = sites.caltech54()
    return infra, Interface({"infrastructure_info": infra, "period": 5})


# ---- the reference's invariants (t_aco.py:50-83) ------------------------------------
def assert_rates_below_max(rates, max_rate, tol=1e-3):
    assert (rates <= max_rate + tol).all()


def energy_delivered(rates, sessions, infrastructure, period):
    out = []
    for s in sessions:
        i = infrastructure.station_ids.index(s.station_id)
        e = rates[i, s.arrival_offset : s.arrival_offset + s.remaining_time].sum()
        out.append(e * infrastructure.voltages[i] * period / 1e3 / 60)
    return np.array(out)


def assert_energy_demands_met(rates, sessions, infrastructure, period):
    delivered = energy_delivered(rates, sessions, infrastructure, period)
    expected = np.array([s.remaining_demand for s in sessions])
    assert np.allclose(delivered, expected, atol=1e-4, rtol=1e-4)


def assert_no_charging_when_unplugged(rates, sessions, infrastructure):
    mask = np.ones(rates.shape, dtype=bool)
    for s in sessions:
        i = infrastructure.station_ids.index(s.station_id)
        mask[i, s.arrival_offset : s.arrival_offset + s.remaining_time] = False
    assert np.allclose(rates[mask], 0)


def infrastructure_violation(rates, infrastructure):
    """max over rows/periods of |[v cos; v sin] @ rates| - limit (utils.py:5-12 formula)."""
    ph = np.deg2rad(infrastructure.phases)
    cm = infrastructure.constraint_matrix
    mag = np.hypot((cm * np.cos(ph)) @ rates, (cm * np.sin(ph)) @ rates)
    return float((mag - np.asarray(infrastructure.constraint_limits)[:, None]).max())


def assert_infrastructure_satisfied(rates, infrastructure, tol=1e-3):
    assert infrastructure_violation(rates, infrastructure) <= tol


# ---- second fixture file: kernel variants and constraint families beyond caltech54 / T = 12 / inequality ----------
WIDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide.npz")


def load_wide():
    return np.load(WIDE, allow_pickle=False)


STALLED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stalled.npz")


def load_stalled():
    """tools/make_golden_stalled.py: certified optima of instances that end the adaptive first pass on a plateau."""
    return np.load(STALLED, allow_pickle=False)


def wide_case(g, name):
    """Rebuild fixture ``name`` of wide.npz / stalled.npz (tools/make_golden_wide.py, make_golden_stalled.py): returns
    (sessions, infrastructure, interface, meta dict, peak_limit, expected dict)."""
    site_tag = str(g[f"{name}_site"])
    infra = sites.eight_sites()[int(site_tag.split(":")[1])] if site_tag.startswith("eight:") else getattr(sites, site_tag)()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    st, arr, dep = g[f"{name}_station"], g[f"{name}_arrival"], g[f"{name}_departure"]
    minr, maxr = g[f"{name}_minr"], g[f"{name}_maxr"]
    sessions, o = [], 0
    for k in range(len(st)):
        L = int(dep[k] - arr[k])
        sessions.append(SessionInfo(infra.station_ids[int(st[k])], f"s{k}", float(g[f"{name}_demand"][k]), 0.0,
                                    int(arr[k]), int(dep[k]), current_time=0,
                                    min_rates=minr[o:o + L].copy(), max_rates=maxr[o:o + L].copy()))
        o += L
    m = g[f"{name}_meta"]
    meta = dict(T=int(m[0]), ct="SOC" if m[1] else "LINEAR", eq=bool(m[2]), es=float(m[3]), seed=int(m[4]))
    pk = g[f"{name}_peak"]
    peak = None if np.isnan(pk[0]) else (float(pk[0]) if len(pk) == 1 else pk.copy())
    exp = dict(rates=g[f"{name}_rates"], obj=float(g[f"{name}_obj"]))
    return sessions, infra, iface, meta, peak, exp


# ---- a minimal closed-loop plant (shape of the reference's integration tests, t_int.py:16-48, without acnsim) --------
def closed_loop_fleet(infra, rng, n_evs=45, t_span=24, stay=(8, 13), fill=(0.5, 0.95), period=5):
    """EV records for a congested closed loop: arrivals over ``t_span`` periods, stays of ``stay`` periods, requests a
    ``fill`` fraction of what the stay could deliver at 32 A."""
    evs = []
    k = infra.voltages[0] * period / 1e3 / 60
    for n, i in enumerate(rng.choice(infra.num_stations, size=n_evs, replace=False)):
        arr = int(rng.integers(0, t_span))
        dur = int(rng.integers(stay[0], stay[1]))
        evs.append(dict(station=infra.station_ids[int(i)], sid=f"ev{n}", arrival=arr, departure=arr + dur,
                        requested=float(rng.uniform(*fill) * 32 * dur * k), delivered=0.0))
    return evs


def closed_loop_sessions(evs, t):
    """SessionInfo list of the EVs plugged in at period ``t`` that still need energy."""
    return [SessionInfo(e["station"], e["sid"], e["requested"], e["delivered"], e["arrival"], e["departure"],
                        current_time=t, max_rates=32.0)
            for e in evs if e["arrival"] <= t < e["departure"] and e["requested"] - e["delivered"] > 1e-9]


def closed_loop_apply(evs, t, first_period_rates, infra, period=5):
    k = infra.voltages[0] * period / 1e3 / 60
    for e in evs:
        if e["arrival"] <= t < e["departure"]:
            r = float(first_period_rates[infra.get_station_index(e["station"])])
            e["delivered"] = min(e["requested"], e["delivered"] + r * k)


PROX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prox.npz")


def load_prox():
    """tools/make_golden_prox.py: certified optima of problems with a load_flattening / demand_charge term at the shapes
    the large-site and the long-horizon kernel serve."""
    return np.load(PROX, allow_pickle=False)


def prox_case(g, name):
    """Rebuild fixture ``name`` of prox.npz: (sessions, infrastructure, interface, objective list, spec for
    oracle/ref_problem.py, meta dict, expected dict)."""
    from adacharge_amd import ObjectiveComponent, demand_charge, equal_share, load_flattening, total_energy

    infra = getattr(sites, str(g[f"{name}_site"]))()
    m = g[f"{name}_meta"]
    meta = dict(T=int(m[0]), ct="SOC" if m[1] else "LINEAR", eq=bool(m[2]), lf=bool(m[3]), seed=int(m[4]),
                es=float(m[5]) if len(m) > 5 else (0.0 if m[3] else 1e-3))
    if meta["lf"]:
        ext = g[f"{name}_ext"].copy()
        obj = [ObjectiveComponent(load_flattening, 1.0, {"external_signal": ext})]
        spec = [("load_flattening", 1.0, {"external_signal": ext})]
        if meta["es"]:
            obj.append(ObjectiveComponent(equal_share, meta["es"]))
            spec.append(("equal_share", meta["es"], {}))
        iface = Interface({"infrastructure_info": infra, "period": 5})
    else:
        obj = [ObjectiveComponent(total_energy, 20.0), ObjectiveComponent(demand_charge), ObjectiveComponent(equal_share, 1e-3)]
        spec = [("total_energy", 20.0, {}), ("demand_charge", 1.0, {}), ("equal_share", 1e-3, {})]
        iface = Interface({"infrastructure_info": infra, "period": 5, "demand_charge": 15.0, "prev_peak": 50.0})
    st, arr, dep = g[f"{name}_station"], g[f"{name}_arrival"], g[f"{name}_departure"]
    minr, maxr = g[f"{name}_minr"], g[f"{name}_maxr"]
    sessions, o = [], 0
    for k in range(len(st)):
        L = int(dep[k] - arr[k])
        sessions.append(SessionInfo(infra.station_ids[int(st[k])], f"s{k}", float(g[f"{name}_demand"][k]), 0.0,
                                    int(arr[k]), int(dep[k]), current_time=0,
                                    min_rates=minr[o:o + L].copy(), max_rates=maxr[o:o + L].copy()))
        o += L
    exp = dict(rates=g[f"{name}_rates"], obj=float(g[f"{name}_obj"]), binding=int(g[f"{name}_binding"][0]))
    return sessions, infra, iface, obj, spec, meta, exp


EDGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edges.npz")


def load_edges():
    """tools/make_golden_edges.py: certified optima at the shape edges of every kernel route."""
    return np.load(EDGES, allow_pickle=False)


def edges_case(g, name):
    """Rebuild fixture ``name`` of edges.npz: (sessions, infrastructure, interface, objective list, meta dict,
    peak_limit, expected dict).  The site is stored with the case (constraint matrix, limits, phases; 208 V, 32 A)."""
    from adacharge_amd import ObjectiveComponent, demand_charge, equal_share, load_flattening, quick_charge, total_energy
    from adacharge_amd.acn import InfrastructureInfo

    cm = g[f"{name}_cm"]
    n = cm.shape[1]
    infra = InfrastructureInfo(cm, g[f"{name}_limits"], g[f"{name}_phases"], np.full(n, 208.0),
                               constraint_ids=[f"c{j}" for j in range(cm.shape[0])], station_ids=[f"E-{i:04d}" for i in range(n)],
                               max_pilot=np.full(n, 32.0), min_pilot=np.full(n, 8.0),
                               allowable_pilots=[np.r_[0.0, np.arange(8.0, 33.0)] for _ in range(n)],
                               is_continuous=np.zeros(n, dtype=bool))
    kind = str(g[f"{name}_objective"])
    if kind == "lf":
        obj = [ObjectiveComponent(load_flattening, 1.0, {"external_signal": g[f"{name}_ext"].copy()}), ObjectiveComponent(equal_share, 1e-3)]
        iface = Interface({"infrastructure_info": infra, "period": 5})
    elif kind == "dc":
        obj = [ObjectiveComponent(total_energy, 20.0), ObjectiveComponent(demand_charge), ObjectiveComponent(equal_share, 1e-3)]
        iface = Interface({"infrastructure_info": infra, "period": 5, "demand_charge": 15.0, "prev_peak": 50.0})
    else:
        obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
        iface = Interface({"infrastructure_info": infra, "period": 5})
    st, arr, dep = g[f"{name}_station"], g[f"{name}_arrival"], g[f"{name}_departure"]
    minr, maxr = g[f"{name}_minr"], g[f"{name}_maxr"]
    sessions, o = [], 0
    for k in range(len(st)):
        L = int(dep[k] - arr[k])
        sessions.append(SessionInfo(infra.station_ids[int(st[k])], f"s{k}", float(g[f"{name}_demand"][k]), 0.0,
                                    int(arr[k]), int(dep[k]), current_time=0,
                                    min_rates=minr[o:o + L].copy(), max_rates=maxr[o:o + L].copy()))
        o += L
    m = g[f"{name}_meta"]
    meta = dict(T=int(m[0]), ct="SOC" if m[1] else "LINEAR", eq=bool(m[2]), seed=int(m[3]), objective=kind,
                family=str(g[f"{name}_family"]), how=str(g[f"{name}_how"]))
    pk = g[f"{name}_peak"]
    peak = None if np.isnan(pk[0]) else (float(pk[0]) if len(pk) == 1 else pk.copy())
    exp = dict(rates=g[f"{name}_rates"], obj=float(g[f"{name}_obj"]), cert=g[f"{name}_cert"])
    return sessions, infra, iface, obj, meta, peak, exp


# ---- padding and certificate pools (oracle/kkt.py; tests/test_kkt_certificate.py, tests/test_route_certificate.py) ----
def pad_batch(batch, t_max, k_sessions):
    """``batch`` padded to ``t_max`` periods and ``k_sessions`` session slots: the same problems (include/acn_qp.h: periods
    t >= horizon[b] are dead -- lb = ub = q = 0, peak = +inf -- and an empty slot has s_len = 0), another padded shape and
    so possibly another kernel family (acnqp_route decides on (t_max, k_sessions), never on horizon[b])."""
    import copy

    assert t_max >= batch.Tm and k_sessions >= batch.K
    B, N, Tm, K = batch.B, batch.N, batch.Tm, batch.K

    def grow(a, shape, fill=0):
        out = np.full(shape, fill, dtype=a.dtype)
        out[tuple(slice(0, s) for s in a.shape)] = a
        return out

    out = copy.copy(batch)
    out.Tm, out.K = int(t_max), int(k_sessions)
    out.lb, out.ub, out.q = (grow(a, (B, N, t_max)) for a in (batch.lb, batch.ub, batch.q))
    out.s_off, out.s_len, out.s_cap = (grow(a, (B, k_sessions, N)) for a in (batch.s_off, batch.s_len, batch.s_cap))
    out.peak = None if batch.peak is None else grow(batch.peak, (B, t_max), np.inf)
    return out


def pad_result(a, t_max):
    """(B, R, Tm) result array padded with zeros to t_max periods (what the library writes at dead periods)"""
    out = np.zeros(a.shape[:-1] + (t_max,), dtype=a.dtype)
    out[..., : a.shape[-1]] = a
    return out


def certificate_pool(site_name, cone, T, n, seed, eq=False, two=True, peak=None):
    """``n`` snapshots of ``site_name`` (sites.random_sessions_general: delayed arrivals, two sessions on 40 % of the
    EVSEs when ``two``), horizons T, T - 2 and T - 4 mixed in one batch; ``peak``: None (no peak row), "scalar",
    "vector" or "mixed" (scalar, vector and unlimited snapshots in one batch)."""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, total_energy
    from adacharge_amd.builder import build_batch

    infra = getattr(sites, site_name)()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(seed)
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3), ObjectiveComponent(total_energy, 0.5)]
    snaps, peaks = [], []
    for k in range(n):
        Tb = T - 2 * (k % 3)
        snaps.append(sites.random_sessions_general(infra, Tb, rng, two_per_evse=two, min_rates=not eq,
                                                   demand_scale=0.5 if eq else 1.5))
        kind = peak if peak != "mixed" else ("scalar", "vector", None)[k % 3]
        Tk = max(s.arrival_offset + s.remaining_time for s in snaps[-1])
        peaks.append(None if kind is None else float(rng.uniform(250, 600)) if kind == "scalar"
                     else rng.uniform(250, 600, size=Tk))
    return build_batch(snaps, infra, iface, obj, cone, eq, peak_limits=peaks if peak else None)


def edges_pool(name, n, seed=0):
    """``n`` demand scenarios (factors U(0.85, 1) per session) of edges.npz case ``name``: its site, horizon and slots."""
    from adacharge_amd.builder import build_batch, scenario_batch

    sl, infra, iface, obj, meta, peak, exp = edges_case(load_edges(), name)
    base = build_batch([sl], infra, iface, obj, meta["ct"], meta["eq"], peak_limits=[peak])
    rng = np.random.default_rng(seed)
    return scenario_batch(base, rng.uniform(0.85, 1.0, size=(n, base.K, base.N)))


# ---- one launch per kernel family (tests/test_route_certificate.py, tests/test_verdicts_gpu.py) -----------------------
T_PADS = (12, 13, 17, 20, 25, 28, 33, 40, 49, 60, 289)


def route_shapes(h, batch):
    """{family: (t_max, k_sessions)}: the smallest padded shape of each family this pool reaches"""
    out = {}
    for k in sorted({batch.K, max(batch.K, 2), 5}):
        for t in sorted({batch.Tm} | {t for t in T_PADS if t >= batch.Tm}):
            fam, _ = h.route(t, k, batch.B)
            out.setdefault(fam, (t, k))
    return out


def poisoned_device_batch(batch):
    """a ``DeviceBatch`` of ``batch`` with every output poisoned: NaN in x, y, pri_res, dua_res and obj, -1 in iters and status"""
    from adacharge_amd.backend import DeviceBatch

    dev = DeviceBatch(batch, "cuda:0", want_y=True)
    for a in (dev.x, dev.y, dev.pri_res, dev.dua_res, dev.obj):
        a.fill_(float("nan"))
    dev.iters.fill_(-1)
    dev.status.fill_(-1)
    return dev


def device_outputs(dev):
    return {k: getattr(dev, k).cpu().numpy() for k in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")}


def launch_poisoned(h, batch, options=None, warm=None):
    """one launch through the device entry with every output poisoned (NaN, iters -1); returns host arrays.
    ``warm = (x0, y0)``: host arrays (B, N, Tm) and (B, Mg, Tm) of a warm start, uploaded as device tensors"""
    import torch

    dev = poisoned_device_batch(batch)
    wx, wy = (None, None) if warm is None else (torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda:0") for a in warm)
    h.solve_device(dev, options, stream=torch.cuda.current_stream().cuda_stream, warm_x=wx, warm_y=wy)
    torch.cuda.synchronize()
    return device_outputs(dev)
