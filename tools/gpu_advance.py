"""Time the advance launch (acnqp_advance_device) at the headline shape, 16,384 x 54 x 12, against the solve launch of the
same batch, and a closed-loop ``simulate_batch`` against the same loop written with ``schedule_batch`` and a Python plant,
all in one process.  The priced launch (acnqp_advance_priced_device, rule 6b: a clock cost) is timed beside the plain one
on the same state, and the closed loop is run once more under a time-of-use tariff.

    python tools/gpu_advance.py [--batch 16384] [--scenarios 256] [--steps 24] [--out profiles/advance_timing.json]

The kernel time is the median of 5 launches between HIP events (one warm-up launch first); the solve time is the sum of
the HIP-event durations of the call's launches (``BatchResult.kernel_ms``); the two loops are one wall-clock run each.
Nothing is asserted about any time.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "advance_timing.json"))
    args = ap.parse_args()

    import torch

    from adacharge_amd import (AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites, total_energy,
                               tou_energy_cost)
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import AdvancePlan, DeviceBatch, default_options
    from adacharge_amd.builder import build_batch_from_table, objective_terms
    from adacharge_amd.adaptive_charging_optimization import _site_handle
    from adacharge_amd.rollout import FleetTable
    from tests import helpers

    infra = sites.caltech54()
    tariff = np.where((np.arange(args.steps + 64) // 4) % 2 == 1, 0.30, 0.06) + 1e-3 * np.arange(args.steps + 64)
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0, "prices": tariff})
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
    N, Tm = batch.N, batch.Tm
    q_table, h_scal = np.zeros((Tm, N, Tm)), np.zeros((Tm, 3))
    for T in range(1, Tm + 1):
        q, pd, lf, _, dc, _ = objective_terms(obj, infra, iface, N, T)
        q_table[T - 1, :, :T], h_scal[T - 1] = q, (pd, lf, dc)
    h_row = np.r_[-1, np.arange(Tm)].astype(np.int32)
    plan = AdvancePlan(q_table, h_scal, h_row, 1e-6, 0.208).to_device(dev)
    series = np.random.default_rng(1).uniform(0.05, 0.4, size=(batch.B, 1 + Tm))
    priced = AdvancePlan(q_table, h_scal, h_row, 1e-6, 0.208, c_coef=1.0, c_weight=np.asarray(infra.voltages, float) / 1e3 * (5 / 60),
                         c_series=series).to_device(dev)
    applied = cur.x[:, :, 0].contiguous()
    flags = torch.empty(batch.B, dtype=torch.int32, device=dev)

    def launch(pl=plan):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        handle.advance_device(cur, nxt, applied, pl, 0, flags)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    launch()
    runs = [launch() for _ in range(5)]
    launch(priced)
    priced_runs = [launch(priced) for _ in range(5)]
    moved = batch.B * (5 * N * Tm * 8 + 2 * batch.K * N * 16 + N * 8)   # lb, ub read; lb', ub', q' written (q_table rows stay in cache)
    # ---- the closed loop ----------------------------------------------------------------------------------------------
    rng = np.random.default_rng(3)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=30, t_span=10, stay=(8, 13)) for _ in range(args.scenarios)]
    alg = AdaptiveSchedulingAlgorithm(obj)
    alg.register_interface(iface)
    records = [[dict(e, max_rate=32.0) for e in f] for f in fleets]
    alg.simulate_batch(records, 2)   # warm-up: handle, allocator
    t0 = time.perf_counter()
    table = FleetTable(records, infra, iface, obj, args.steps)
    t1 = time.perf_counter()
    res = alg.simulate_batch(table, args.steps)
    device_s = time.perf_counter() - t1
    # the same loop under a time-of-use tariff (the priced advance at every step)
    tou = AdaptiveSchedulingAlgorithm([ObjectiveComponent(total_energy, 0.15), ObjectiveComponent(equal_share, 1e-12), ObjectiveComponent(tou_energy_cost)])
    tou.register_interface(iface)
    tou.simulate_batch(records, 2)
    t2 = time.perf_counter()
    tou_table = FleetTable(records, infra, iface, tou.objective, args.steps)
    t3 = time.perf_counter()
    tou_res = tou.simulate_batch(tou_table, args.steps)
    tou_s = time.perf_counter() - t3
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
        "shape": [int(batch.B), int(N), int(Tm)],
        "device": torch.cuda.get_device_name(dev),
        "advance_launch_ms": {"median": statistics.median(runs), "runs": runs},
        "advance_gb_per_s": moved / statistics.median(runs) / 1e6,
        "advance_priced_launch_ms": {"median": statistics.median(priced_runs), "runs": priced_runs},
        "advance_priced_gb_per_s": moved / statistics.median(priced_runs) / 1e6,
        "solve_launch_ms": solve_ms,
        "closed_loop": {"scenarios": args.scenarios, "steps": args.steps, "fleet_table_s": table_s, "simulate_batch_s": device_s,
                        "schedule_batch_and_python_plant_s": host_s,
                        "delivered_fraction_device": float(sum(d.sum() for d in res.delivered) / requested),
                        "delivered_fraction_host": float(sum(e["delivered"] for f in fleets for e in f) / requested),
                        "flags": int(np.count_nonzero(res.flags)), "not_solved": int((~np.isin(res.status, (1, 5))).sum())},
        "closed_loop_tou": {"scenarios": args.scenarios, "steps": args.steps, "fleet_table_s": t3 - t2, "simulate_batch_s": tou_s,
                            "energy_cost_total": float(tou_res.energy_cost.sum()), "flags": int(np.count_nonzero(tou_res.flags)),
                            "not_solved": int((~np.isin(tou_res.status, (1, 5))).sum())},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
