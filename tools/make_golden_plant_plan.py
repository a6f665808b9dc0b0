"""Write tests/golden/plant_parent_plan.npz: everything ``rollout.FleetTable`` precomputes for a small fleet WITHOUT batteries
(three scenarios of caltech54, eight steps, a peak limit, arrival order).  It was run on the commit before the plant entries
existed; tests/test_plant_spec.py rebuilds the same table and holds every array to the file, so that a fleet without
batteries keeps building the plan it always built.

    python tools/make_golden_plant_plan.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table():
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.rollout import FleetTable
    from tests import helpers

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    rng = np.random.default_rng(2024)
    fleets = [[dict(e, max_rate=32.0, min_rate=0.0 if n % 3 else 6.0) for n, e in enumerate(helpers.closed_loop_fleet(infra, rng, n_evs=12, t_span=6, stay=(3, 7)))]
              for _ in range(3)]
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    return FleetTable(fleets, infra, iface, obj, steps=8, t_max=6, peak_limit=300.0, session_order="arrival")


def arrays(t):
    out = {k: np.asarray(getattr(t.plan, k)) for k in t.plan._ARRAYS if getattr(t.plan, k) is not None}
    out.update(done_tol=np.float64(t.plan.done_tol), kw_per_amp=np.float64(t.plan.kw_per_amp), dfloor0=np.float64(t.dfloor0),
               order_keys=t.order_keys, min_pilot=t.min_pilot, kwh_per_amp_period=t.kwh_per_amp_period)
    return {k: np.asarray(v) for k, v in out.items()}


if __name__ == "__main__":
    path = os.path.join(ROOT, "tests", "golden", "plant_parent_plan.npz")
    np.savez_compressed(path, **arrays(table()))
    print(path, os.path.getsize(path), "bytes")
