"""Generates tests/golden/edges.npz: oracle-certified optima at the shape edges of every kernel route.

The library picks one of its kernel families per launch by shape alone (wave_shape, tiled_shape, lds_long_shape,
stream_shape, long_shape and route_for in acn_qp_route.hpp): cut points at N 64/65, horizons 12/13,
16/17, 24/25, 32/33, 48/49 and 288/289, 16/32/48 padded site rows (SOC pads its 2M rows to 8 ceil(M/4)) and four
session slots per EVSE.  Each case below sits on one side of such a cut and records the family it is written for;
tests/test_golden_edges.py checks on the GPU that acnqp_route agrees, so that a later routing change cannot quietly
move a case off its edge.  Padded lanes (N not a multiple of 16 / 64), dead period registers and partial MFMA tiles
are what these cases exercise.

Table notes (where the routing differs from a naive reading of the shape):
  - five sessions on one EVSE (over kMaxK = 4) leave the tiled kernel for the long-horizon kernel's WORKSPACE variant
    (the LDS variant needs two row tiles, MR = 32);
  - N = 64 x 49 and N = 65 x 49 LINEAR (one row tile) run the long-horizon kernel's workspace variant (the LDS variant
    is for horizons 17-32).

Sites: caltech54 / jpl52 by name, `sites.balanced_three_phase(n, pods)` otherwise, and a one-feeder single-phase site
for N = 1 and N = 4 (LINEAR: one row).  The site's rows (constraint matrix, limits, phases) are stored with the case.
Objective: quick_charge + equal_share * 1e-3 (strictly convex) unless `obj` says `lf` (load_flattening of an external
profile -- an export, so that flattening means charging -- + equal_share * 1e-3; the IPM stops at its reduced-accuracy exit there, so the certified point is reached from
the C twin's answer by the active-set Newton of oracle/ipm.py -- `how` = twin+polish) or `dc` (total_energy +
demand_charge + equal_share * 1e-3, BASELINE-style demand charge of 15 with a previous peak of 50).  Every certificate
is the KKT check of oracle/ipm.py on the full problem oracle/ref_problem.py states, <= 1e-9.

    python tools/make_golden_edges.py [name ...]   (re)generate these cases (default: all), keep the others
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from adacharge_amd import sites
from adacharge_amd.acn import InfrastructureInfo, Interface, SessionInfo

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "edges.npz")


def single_phase(n, frac=0.6):
    """n EVSEs on one feeder (one row, phase 0) rated at `frac` of their full load"""
    return InfrastructureInfo(np.ones((1, n)), np.array([frac * 32.0 * n]), np.zeros(n), np.full(n, 208.0),
                              constraint_ids=["feeder"], station_ids=[f"SP-{i:04d}" for i in range(n)],
                              max_pilot=np.full(n, 32.0), min_pilot=np.full(n, 8.0),
                              allowable_pilots=[np.r_[0.0, np.arange(8.0, 33.0)] for _ in range(n)],
                              is_continuous=np.zeros(n, dtype=bool))


def site_of(spec):
    if spec == "caltech54":
        return sites.caltech54()
    if spec == "jpl52":
        return sites.jpl52()
    kind, n, pods = spec
    if kind == "single":
        return single_phase(n)
    return sites.balanced_three_phase(n, pods=pods, load_fraction=0.35, name=f"E{n}")


# name: (site, T, cone, energy equality, min rates, peak ("none" | "scalar" | "vector"), objective ("qc" | "lf" | "dc"),
#        sessions on the busiest EVSE (consecutive windows), at most this many sessions (None: N/3 .. N), seed, family)
CASES = {
    "n1_t1":          (("single", 1, 0),  1,   "LINEAR", False, False, "none",   "qc", 1, None, 301, "wave1"),
    "n17_t12_soc":    (("b3p", 17, 2),    12,  "SOC",    False, True,  "none",   "qc", 1, None, 302, "wave1"),
    "ct54_t13":       ("caltech54",       13,  "SOC",    False, False, "none",   "qc", 1, None, 303, "wave2"),
    "ct54_t25_soc":   ("caltech54",       25,  "SOC",    False, True,  "none",   "qc", 1, None, 304, "tiled_ct2"),
    "ct54_t32_lin_eq": ("caltech54",      32,  "LINEAR", True,  False, "none",   "qc", 1, None, 305, "tiled_ct2"),
    "ct54_t33_soc":   ("caltech54",       33,  "SOC",    False, False, "none",   "qc", 1, None, 306, "wave5"),
    "ct54_t48_lin_vpeak": ("caltech54",   48,  "LINEAR", False, True,  "vector", "qc", 1, None, 307, "wave5"),
    "ct54_t12_soc_speak": ("caltech54",   12,  "SOC",    False, False, "scalar", "qc", 1, None, 308, "wave3"),
    "jpl_t13_soc":    ("jpl52",           13,  "SOC",    False, True,  "none",   "qc", 1, None, 309, "wave4"),
    "jpl_t25_soc":    ("jpl52",           25,  "SOC",    False, False, "none",   "qc", 1, None, 310, "long_lds"),
    "jpl_t32_soc_eq": ("jpl52",           32,  "SOC",    True,  False, "none",   "qc", 1, None, 311, "long_lds"),
    "jpl_t28_dc":     ("jpl52",           28,  "SOC",    False, False, "none",   "dc", 1, None, 312, "long_ws"),
    "ct54_t16_k4":    ("caltech54",       16,  "SOC",    False, False, "none",   "qc", 4, None, 313, "tiled_ct1"),
    "ct54_t16_k5":    ("caltech54",       16,  "SOC",    False, False, "none",   "qc", 5, None, 314, "long_ws"),
    "n60_t16_soc_peak": (("b3p", 60, 8),  16,  "SOC",    False, True,  "scalar", "qc", 1, None, 315, "tiled_ct1"),
    "n60_t17_soc_peak": (("b3p", 60, 8),  17,  "SOC",    False, False, "scalar", "qc", 1, None, 316, "general"),
    "n64_t49_lin":    (("b3p", 64, 4),    49,  "LINEAR", False, False, "none",   "qc", 1, None, 317, "long_ws"),
    "n4_t289":        (("single", 4, 0),  289, "LINEAR", False, False, "none",   "qc", 1, None, 318, "general"),
    "n65_t1":         (("b3p", 65, 4),    1,   "SOC",    False, False, "none",   "qc", 1, None, 319, "stream"),
    "n65_t16_lin":    (("b3p", 65, 4),    16,  "LINEAR", False, True,   "none",   "qc", 1, None, 320, "stream"),
    "n79_t17_soc":    (("b3p", 79, 4),    17,  "SOC",    False, True,  "vector", "qc", 1, None, 321, "stream"),
    "n100_t33_soc":   (("b3p", 100, 12),  33,  "SOC",    False, False, "none",   "qc", 1, None, 322, "stream"),
    "n100_t24_lf":    (("b3p", 100, 4),   24,  "SOC",    False, False, "none",   "lf", 1, 40,   323, "stream"),
    "n1023_t12_soc":  (("b3p", 1023, 12), 12,  "SOC",    False, False, "none",   "qc", 1, 160,  324, "stream"),
    "n65_t49_lin":    (("b3p", 65, 4),    49,  "LINEAR", False, False, "none",   "qc", 1, None, 325, "long_ws"),
    "n65_t49_soc":    (("b3p", 65, 12),   49,  "SOC",    False, False, "none",   "qc", 1, None, 326, "general"),
}


def sessions_for(infra, T, rng, mins, k_busy, max_sessions, eq):
    """sessions of one snapshot whose own horizon is exactly T: S EVSEs (N/3 .. N, at most `max_sessions`), arrival in
    the first third, the first session staying to T; `k_busy` consecutive sessions on the first EVSE; stepped maximum
    rates on a fifth of the sessions, minimum rates (6 A over a prefix) on 30 % of them when `mins`"""
    n = infra.num_stations
    s = int(rng.integers(max(1, n // 3), n + 1))
    if max_sessions:
        s = min(s, max_sessions)
    evses = rng.choice(n, size=s, replace=False)
    out = []
    for j, i in enumerate(evses):
        sid = infra.station_ids[int(i)]
        kwh = float(infra.voltages[int(i)]) * 5 / 60 / 1e3
        if j == 0 and k_busy > 1:
            cuts = np.linspace(0, T, k_busy + 1).astype(int)
            spans = [(int(cuts[m]), int(cuts[m + 1]) - (1 if m < k_busy - 1 else 0)) for m in range(k_busy)]
        else:
            a = 0 if j == 0 else int(rng.integers(0, max(1, T // 3)))
            spans = [(a, T if j == 0 else int(rng.integers(a + 1, T + 1)))]
        for m, (a, d) in enumerate(spans):
            L = d - a
            lo = np.zeros(L)
            if mins and rng.random() < 0.3:
                lo[: int(rng.integers(1, L + 1))] = 6.0
            hi = np.full(L, 32.0)
            if rng.random() < 0.2:
                hi[int(rng.integers(0, L)):] = 16.0
            dem = float(rng.uniform(0.2, 1.0) * (0.5 if eq else 1.5) * 32 * L * kwh)
            dem = max(dem, lo.sum() * kwh + 0.01)
            if eq:
                dem = min(dem, 0.9 * hi.sum() * kwh)
            out.append(SessionInfo(sid, f"{sid}-{m}", dem, 0.0, a, d, current_time=0, min_rates=lo, max_rates=hi))
    return out


def objective_of(kind, T):
    """(spec for oracle/ref_problem.py, ObjectiveComponent list for the builder, Interface settings, external profile)"""
    from adacharge_amd import ObjectiveComponent, demand_charge, equal_share, load_flattening, quick_charge, total_energy

    if kind == "lf":
        # a NEGATIVE external load (export of 50-250 kW): flattening it means charging, so the optimum is not the zero
        # schedule (a positive profile with inequality demands makes it zero)
        ext = -100.0 * (1.5 + np.cos(np.arange(T) / T * 2 * np.pi))
        return ([("load_flattening", 1.0, {"external_signal": ext}), ("equal_share", 1e-3, {})],
                [ObjectiveComponent(load_flattening, 1.0, {"external_signal": ext}), ObjectiveComponent(equal_share, 1e-3)], {}, ext)
    if kind == "dc":
        return ([("total_energy", 20.0, {}), ("demand_charge", 1.0, {}), ("equal_share", 1e-3, {})],
                [ObjectiveComponent(total_energy, 20.0), ObjectiveComponent(demand_charge), ObjectiveComponent(equal_share, 1e-3)],
                {"demand_charge": 15.0, "prev_peak": 50.0}, np.zeros(0))
    return ([("quick_charge", 1, {}), ("equal_share", 1e-3, {})],
            [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)], {}, np.zeros(0))


def case_problem(name):
    site, T, ct, eq, mins, peak_kind, kind, k_busy, max_s, seed, family = CASES[name]
    infra = site_of(site)
    rng = np.random.default_rng(seed)
    sl = sessions_for(infra, T, rng, mins, k_busy, max_s, eq)
    assert max(s.arrival_offset + s.remaining_time for s in sl) == T
    full = 32.0 * len(sl)
    peak = None
    if peak_kind == "scalar":
        peak = float(rng.uniform(0.25, 0.5) * full)
    elif peak_kind == "vector":
        peak = rng.uniform(0.25, 0.6, size=T) * full
    if peak is not None:   # the peak must leave the minimum rates feasible
        lbsum = np.zeros(T)
        for s in sl:
            lbsum[s.arrival_offset:s.arrival_offset + s.remaining_time] += s.min_rates
        peak = np.maximum(peak, lbsum + 1.0) if peak_kind == "vector" else max(peak, float(lbsum.max()) + 1.0)
    spec, obj, extra, ext = objective_of(kind, T)
    iface = Interface({"infrastructure_info": infra, "period": 5, **extra})
    return infra, iface, sl, spec, obj, ext, peak


def main():
    from oracle.ipm import solve_certified
    from oracle.ref_problem import build_reference_problem

    only = sys.argv[1:] or list(CASES)
    for name in only:
        site, T, ct, eq, mins, peak_kind, kind, k_busy, max_s, seed, family = CASES[name]
        infra, iface, sl, spec, obj, ext, peak = case_problem(name)
        t0 = time.time()
        prob = build_reference_problem(sl, infra, iface, spec, ct, eq, peak_limit=peak)
        how, r, cert = "ipm", None, None
        if kind != "lf":
            r, _, cert = solve_certified(prob)
        if cert is None or not cert.worst < 1e-9:
            # make_golden_prox.py: the certificate on the full problem, not the path to the point, makes it an oracle value
            from adacharge_amd.builder import build_batch
            from oracle import admm_port
            from oracle.ipm import polish

            batch = build_batch([sl], infra, iface, obj, ct, eq, peak_limits=[peak])
            tw = admm_port.solve_batch(batch, eps_abs=1e-10, eps_rel=1e-10, max_iter=200000, accel_mem=5)
            assert tw["status"][0] == 1, (name, tw["status"], tw["iters"])
            r, cert = polish(prob, tw["x"][0][:, :prob.T], duals=None, act_tol=1e-6, max_rounds=60)
            r = prob.rates_of(r)
            how = "twin+polish"
        assert cert is not None and cert.worst < 1e-9, (name, cert)
        st = {
            "cm": infra.constraint_matrix, "limits": infra.constraint_limits, "phases": infra.phases,
            "station": np.array([infra.station_ids.index(s.station_id) for s in sl], np.int32),
            "arrival": np.array([s.arrival for s in sl], np.int32),
            "departure": np.array([s.departure for s in sl], np.int32),
            "demand": np.array([s.remaining_demand for s in sl]),
            "minr": np.concatenate([s.min_rates for s in sl]),
            "maxr": np.concatenate([s.max_rates for s in sl]),
            "peak": np.array([np.nan]) if peak is None else np.atleast_1d(np.asarray(peak, float)),
            "meta": np.array([T, 1 if ct == "SOC" else 0, 1 if eq else 0, seed], float),
            "objective": np.array(kind), "ext": ext, "family": np.array(family), "how": np.array(how),
            "rates": r,
            "obj": np.array(prob.objective(r)),
            "cert": np.array([cert.stationarity, cert.primal, cert.dual]),
        }
        store = dict(np.load(OUT, allow_pickle=False)) if os.path.exists(OUT) else {}
        for k, v in st.items():
            store[f"{name}_{k}"] = v
        store["names"] = np.array([n for n in CASES if f"{n}_rates" in store])
        np.savez_compressed(OUT, **store)
        K = int(np.bincount(st["station"]).max())
        print(f"{name:20s} N={infra.num_stations:4d} T={T:3d} {ct:6s} eq={int(eq)} K={K} S={len(sl):3d} peak={peak_kind:6s} "
              f"{kind} {family:9s} obj {prob.objective(r):.9f} cert {cert.worst:.1e} ({how})  {time.time() - t0:.1f}s", flush=True)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
