"""Cases for the wave kernel's EVSE extent (acn_qp_rank.hpp).  Run as a
script it solves EVERY case under the environment it was started with (ACNQP_WAVE_FULL_EVSE=1: P = Ghat r0 over all 16
EVSE k-steps; ACNQP_LIBRARY: another build of the library) and saves the results; without ``--results-only`` also what
acnqp_debug_wave_evse_extent reports for each handle and the route.  tests/test_wave_trim_gpu.py compares such runs with
each other and with tests/golden/wave_trim.npz (tools/make_golden_wave_trim.py: the same cases on the parent's library).

What the cases are for:
  c54_h12    caltech54, horizon 12: one wave per problem; N = 54, so the last live EVSE k-step (13) is half padding
  jpl52_h24  the 52-EVSE site, horizon 24: two row tiles, four waves per problem
  c54_h24    caltech54, horizon 24: two waves per problem
  s36_h12    a 36-EVSE site of BASELINE.json configs[3]: two row tiles, two waves per problem
  syn56      56 EVSEs on 8 disjoint feeders: the largest site of extent 14
  syn57      57 EVSEs: the smallest site that keeps all 16 k-steps
  warm       caltech54, horizon 12, started from a perturbed solution with its multipliers
Every case holds a problem of >= 60 iterations (the Anderson ring of 5 slots, one event per 5 iterations, then wraps:
every slot is written twice) and a problem that adapts rho, which restarts the ring (tools/make_golden_wave_trim.py
--check-twin asserts both on the CPU twin): the golden file pins the whole iteration, the Anderson event included."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = ("c54_h12", "jpl52_h24", "c54_h24", "s36_h12", "syn56", "syn57", "warm")
BATCH = {"jpl52_h24": 8, "c54_h24": 8}   # (the others: 16; the golden file stays at a few hundred KB)
KEYS = ("x", "status", "iters", "pri_res", "dua_res", "obj")
FAMILY = {"c54_h12": "wave1", "jpl52_h24": "wave4", "c54_h24": "wave2", "s36_h12": "wave3", "syn56": "wave1", "syn57": "wave1", "warm": "wave1"}


def build(name):
    """(batch, solve keywords)"""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch
    from tests.wave_rank_cases import disjoint_site

    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    seed = 9100 + CASES.index(name)
    B = BATCH.get(name, 16)
    if name.startswith("syn"):
        infra = disjoint_site(8, n=int(name[3:]))
        iface = Interface({"infrastructure_info": infra, "period": 5})
        return build_batch(sites.snapshot_batch(infra, 12, B, seed=seed), infra, iface, obj, "LINEAR"), {}
    infra = {"jpl52_h24": sites.jpl52, "s36_h12": lambda: sites.eight_sites()[3]}.get(name, sites.caltech54)()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    T = 24 if name.endswith("_h24") else 12
    batch = build_batch(sites.snapshot_batch(infra, T, B, seed=seed), infra, iface, obj, "SOC")
    return batch, (dict(warm="self") if name == "warm" else {})


def solve(name, results_only=False):
    from adacharge_amd.backend import SiteHandle, default_options

    batch, skw = build(name)
    h = SiteHandle(batch.site, 0)
    opts = default_options()
    warm = None
    if skw.get("warm") == "self":
        first = h.solve(batch, opts, want_y=True)
        warm = (first.x * np.random.default_rng(5).uniform(0.9, 1.0, size=first.x.shape), first.y)
    res = h.solve(batch, opts, warm=warm)
    out = dict(x=res.x, status=res.status, iters=res.iters, pri_res=res.pri_res, dua_res=res.dua_res, obj=res.obj)
    if not results_only:
        info = h.wave_evse_extent()
        out.update(n_evse=info["n_evse"], evse_ksteps=info["evse_ksteps"], extent=info["extent"], family=h.route(batch.Tm, batch.K, batch.B)[0])
    h.close()
    return out


if __name__ == "__main__":
    flat = {}
    for name in CASES:
        for k, v in solve(name, "--results-only" in sys.argv[2:]).items():
            flat[f"{name}:{k}"] = v
    np.savez_compressed(sys.argv[1], **flat)
