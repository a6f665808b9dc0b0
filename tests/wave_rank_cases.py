"""Cases for the wave kernel's eigen extent (acn_qp_rank.hpp), 32 problems each.  Run as a script it
solves EVERY case under the environment it was started with (ACNQP_WAVE_FULL_RANK=1: the full extent on the shared
eigenbasis -- the kernel as it was; unset: the site's own extent on the compacted eigenbasis) and saves the results and
what acnqp_debug_wave_rank reports for each handle.  tests/test_wave_rank_gpu.py compares the two runs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B = 32
SYNTHETIC_ROWS = (8, 9, 12, 13, 16)   # rank = rows: the extents' 4-row boundaries; 13 and 16 take the full extent
CASES = ("soc_h12", "linear_h12", "soc_h24", "soc_h40", "mt2_h12", "mt2_h24", "infeasible", "warm") + tuple(f"syn{m}" for m in SYNTHETIC_ROWS)
KEYS = ("status", "iters", "x", "pri", "dua", "obj")


def disjoint_site(rows, n=32):
    """LINEAR site of ``rows`` feeders with disjoint EVSE supports: G G' is diagonal and of full rank."""
    from adacharge_amd.acn import InfrastructureInfo

    cm = np.zeros((rows, n))
    for j, members in enumerate(np.array_split(np.arange(n), rows)):
        cm[j, members] = 1.0
    limits = 20.0 * cm.sum(axis=1)   # 20 A per EVSE of the feeder: binds whenever most of its EVSEs charge at once
    return InfrastructureInfo(cm, limits, np.zeros(n), np.full(n, 208.0), constraint_ids=[f"f{j}" for j in range(rows)],
                              station_ids=[f"DJ-{i:02d}" for i in range(n)], max_pilot=np.full(n, 32.0), min_pilot=np.full(n, 8.0),
                              allowable_pilots=[np.r_[0.0, np.arange(8.0, 33.0)] for _ in range(n)], is_continuous=np.zeros(n, dtype=bool))


def build(name):
    """(batch, options keywords, solve keywords)"""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch
    from adacharge_amd.sites import SessionInfo

    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    seed = 7000 + CASES.index(name)
    if name.startswith("syn"):
        infra = disjoint_site(int(name[3:]))
        iface = Interface({"infrastructure_info": infra, "period": 5})
        snaps = sites.snapshot_batch(infra, 3, B, seed=seed, demand_range=(0.5, 3.0))
        return build_batch(snaps, infra, iface, obj, "LINEAR"), {}, dict(want_y=True)
    infra = sites.eight_sites()[3] if name.startswith("mt2") else sites.caltech54()   # eight_sites()[3]: 36 EVSEs, 18 rows -- two row tiles
    iface = Interface({"infrastructure_info": infra, "period": 5})
    if name == "infeasible":   # energy equalities; problem 0 asks more of every EVSE than the site's feeders carry in an hour
        rng = np.random.default_rng(seed)
        snaps = []
        for b in range(B):
            n = infra.num_stations if b == 0 else int(rng.integers(6, 30))
            evses = rng.choice(infra.num_stations, size=n, replace=False)
            snaps.append([SessionInfo(infra.station_ids[int(e)], f"s{k}", 6.0 if b == 0 else float(rng.uniform(1.0, 3.0)), 0.0, 0, 12,
                                      current_time=0, min_rates=np.zeros(12), max_rates=32.0) for k, e in enumerate(evses)])
        return build_batch(snaps, infra, iface, obj, "SOC", True), dict(max_iter=30000), {}
    if name == "warm":
        return build_batch(sites.snapshot_batch(infra, 12, B, seed=seed), infra, iface, obj, "SOC"), {}, dict(warm="self", want_y=True)
    T = int(name.split("_h")[1])
    ct = "LINEAR" if name.startswith("linear") else "SOC"
    return build_batch(sites.snapshot_batch(infra, T, B, seed=seed), infra, iface, obj, ct), {}, {}


def solve(name):
    from adacharge_amd.backend import SiteHandle, default_options

    batch, okw, skw = build(name)
    h = SiteHandle(batch.site, 0)
    opts = default_options(**okw)
    warm = None
    if skw.get("warm") == "self":
        first = h.solve(batch, opts, want_y=True)
        warm = (first.x * np.random.default_rng(5).uniform(0.9, 1.0, size=first.x.shape), first.y)
    res = h.solve(batch, opts, warm=warm, want_y=bool(skw.get("want_y")))
    info = h.wave_rank()
    out = dict(x=res.x, iters=res.iters, status=res.status, pri=res.pri_res, dua=res.dua_res, obj=res.obj,
               rank=info["rank"], eig_ksteps=info["eig_ksteps"], extent=info["extent"], family=h.route(batch.Tm, batch.K, batch.B)[0])
    if res.y is not None:
        out["y"] = res.y
    h.close()
    return out


if __name__ == "__main__":
    flat = {}
    for name in CASES:
        for k, v in solve(name).items():
            flat[f"{name}:{k}"] = v
    np.savez(sys.argv[1], **flat)
