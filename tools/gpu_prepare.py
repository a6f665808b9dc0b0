"""Time the prepare launch (acnqp_prepare_device, minimum rates and view both on) at the headline shape, 16,384 x 54 x 12,
beside the advance launch and the solve launch of the same batch, and a closed-loop ``simulate_batch`` with
``uninterrupted_charging``, ``quantize`` and ``reallocate`` against the same loop written with ``schedule_batch`` and a Python
plant, all in one process.

    python tools/gpu_prepare.py [--batch 16384] [--scenarios 256] [--steps 24] [--out profiles/prepare_timing.json]

The kernel times are the median of 5 launches between HIP events (one warm-up launch first); the solve time is the sum of
the HIP-event durations of the call's launches; the two loops are one wall-clock run each.  The prepare launch is timed
three ways -- walk and view, the view alone, the walk alone -- so that the figure says which phase costs what.  Nothing is
asserted about any time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_timing.json"))
    args = ap.parse_args()

    import torch

    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import AdvancePlan, DeviceBatch, PreparePlan, default_options
    from adacharge_amd.builder import build_batch_from_table, objective_terms
    from adacharge_amd.adaptive_charging_optimization import _site_handle
    from adacharge_amd.rollout import FleetTable
    from tests import helpers

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    # ---- one launch at the headline shape ----------------------------------------------------------------------------
    batch = build_batch_from_table(sites.snapshot_table(infra, args.horizon, args.batch), infra, iface, obj)
    site, handle = _site_handle(infra, "SOC", False, 0)
    dev = torch.device("cuda", 0)
    cur = DeviceBatch(batch, dev)
    nxt = DeviceBatch.empty(site, batch.B, batch.Tm, batch.K, dev)
    handle.kernel_times()
    handle.solve_device(cur, default_options())
    torch.cuda.synchronize(dev)
    solve_ms = float(sum(handle.kernel_times()))
    B, N, Tm = batch.B, batch.N, batch.Tm
    q_table, h_scal = np.zeros((Tm, N, Tm)), np.zeros((Tm, 3))
    for T in range(1, Tm + 1):
        q, pd, lf, _, dc, _ = objective_terms(obj, infra, iface, N, T)
        q_table[T - 1, :, :T], h_scal[T - 1] = q, (pd, lf, dc)
    plan = AdvancePlan(q_table, h_scal, np.r_[-1, np.arange(Tm)].astype(np.int32), 1e-6, 0.208).to_device(dev)
    applied = cur.x[:, :, 0].contiguous()
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    cm, ph = infra.constraint_matrix, np.deg2rad(infra.phases)
    rng = np.random.default_rng(1)
    keys = np.argsort(rng.random((B, N)), axis=1).astype(np.int32)        # a random list order per problem
    pplan = PreparePlan(key=keys, cre=np.ascontiguousarray(cm * np.cos(ph)), cim=np.ascontiguousarray(cm * np.sin(ph)),
                        limits=np.ascontiguousarray(infra.constraint_limits, float), min_pilot=np.asarray(infra.min_pilot, float)).to_device(dev)
    view = [torch.empty((B, N), dtype=dt, device=dev) for dt in (torch.int32, torch.uint8, torch.float64)]
    present = int(((batch.s_len[:, 0] > 0) & (batch.s_off[:, 0] == 0)).sum())

    def timed(call):
        def once():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        once()
        runs = [once() for _ in range(5)]
        return {"median": statistics.median(runs), "runs": runs}

    advance = timed(lambda: handle.advance_device(cur, nxt, applied, plan, 0, flags))
    # (the walk is idempotent on its own output: a second launch accepts and refuses the same sessions)
    both = timed(lambda: handle.prepare_device(cur, pplan, flags, *view))
    view_only = timed(lambda: handle.prepare_device(cur, pplan, flags, *view, min_rates=False))
    walk_only = timed(lambda: handle.prepare_device(cur, pplan, flags))
    # ---- the closed loop with all three settings --------------------------------------------------------------------------
    rng = np.random.default_rng(3)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=30, t_span=10, stay=(8, 13)) for _ in range(args.scenarios)]
    kw = dict(uninterrupted_charging=True, quantize=True, reallocate=True)
    alg = AdaptiveSchedulingAlgorithm(obj, **kw)
    alg.register_interface(iface)
    records = [[dict(e, max_rate=32.0) for e in f] for f in fleets]
    alg.simulate_batch(records, 2, session_order="fleet")   # warm-up: handle, allocator
    t0 = time.perf_counter()
    table = FleetTable(records, infra, iface, obj, args.steps, session_order="fleet")
    t1 = time.perf_counter()
    res = alg.simulate_batch(table, args.steps, session_order="fleet")
    device_s = time.perf_counter() - t1
    t0, table_s = time.perf_counter(), t1 - t0
    for t in range(args.steps):
        iface.data["current_time"] = t
        lists = [helpers.closed_loop_sessions(f, t) for f in fleets]
        if any(lists):
            rates, _ = alg.schedule_batch(lists, as_arrays=True, postprocess="device", first_period_only=True)
            for b, f in enumerate(fleets):
                helpers.closed_loop_apply(f, t, rates[b], infra)
    host_s = time.perf_counter() - t0
    requested = sum(e["requested"] for f in fleets for e in f)
    out = {
        "shape": [int(B), int(N), int(Tm)],
        "device": torch.cuda.get_device_name(dev),
        "present_sessions_per_problem": present / B,
        "prepare_launch_ms": both,
        "prepare_view_only_ms": view_only,
        "prepare_walk_only_ms": walk_only,
        "advance_launch_ms": advance,
        "solve_launch_ms": solve_ms,
        "prepare_over_solve": both["median"] / solve_ms,
        "closed_loop": {"settings": sorted(kw), "session_order": "fleet", "scenarios": args.scenarios, "steps": args.steps,
                        "fleet_table_s": table_s, "simulate_batch_s": device_s, "schedule_batch_and_python_plant_s": host_s,
                        "delivered_fraction_device": float(sum(d.sum() for d in res.delivered) / requested),
                        "delivered_fraction_host": float(sum(e["delivered"] for f in fleets for e in f) / requested),
                        "flags": int(np.count_nonzero(res.flags)), "prepare_flags": int(np.count_nonzero(res.prepare_flags)),
                        "visits_total": int(res.visits.sum()), "not_solved": int((~np.isin(res.status, (1, 5))).sum())},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
