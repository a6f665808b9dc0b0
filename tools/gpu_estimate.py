"""Time the estimator launch (acnqp_estimate_device) at 16,384 x 54 beside the advance launch (acnqp_advance_device) of the
same batch at Tm = 12, and a closed-loop ``simulate_batch`` of 256 scenarios x 30 EVs x 24 steps with a battery per EV and
``estimate_max_rate=True`` against the same loop without the estimator, all in one process.

    python tools/gpu_estimate.py [--batch 16384] [--scenarios 256] [--steps 24] [--out profiles/estimate_timing.json]

A launch time is the median of 5 launches between HIP events (one warm-up launch first); a loop is the median of 3
wall-clock runs after a warm-up run.  Nothing is asserted about any time.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "estimate_timing.json"))
    args = ap.parse_args()

    import torch

    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, SimpleRampdown, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.adaptive_charging_optimization import _site_handle
    from adacharge_amd.backend import AdvancePlan, DeviceBatch, default_options
    from adacharge_amd.builder import build_batch_from_table, objective_terms
    from adacharge_amd.rollout import FleetTable
    from gpu_plant import battery
    from tests import helpers

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev)}

    def median_launch(launch):
        def once():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        once()
        runs = [once() for _ in range(5)]
        return {"median": statistics.median(runs), "runs": runs}

    # ---- one launch of either kernel on the same solved batch ----------------------------------------------------------
    batch = build_batch_from_table(sites.snapshot_table(infra, args.horizon, args.batch), infra, iface, obj)
    site, handle = _site_handle(infra, "SOC", False, 0)
    cur = DeviceBatch(batch, dev)
    nxt = DeviceBatch.empty(site, batch.B, batch.Tm, batch.K, dev)
    handle.solve_device(cur, default_options())
    torch.cuda.synchronize(dev)
    Bn, N, Tm = batch.B, batch.N, batch.Tm
    q_table, h_scal = np.zeros((Tm, N, Tm)), np.zeros((Tm, 3))
    for T in range(1, Tm + 1):
        q, pd, lf, _, dc, _ = objective_terms(obj, infra, iface, N, T)
        q_table[T - 1, :, :T], h_scal[T - 1] = q, (pd, lf, dc)
    plan = AdvancePlan(q_table, h_scal, np.r_[-1, np.arange(Tm)].astype(np.int32), 1e-6, 0.208).to_device(dev)
    applied = cur.x[:, :, 0].contiguous()
    flags = torch.empty(Bn, dtype=torch.int32, device=dev)
    out["advance_launch_ms"] = median_launch(lambda: handle.advance_device(cur, nxt, applied, plan, 0, flags))
    # the history: a third of the EVs drew 3 A less than offered (ramp down), the rest what they were offered; one slot in
    # eight is seen for the first time
    rng = np.random.default_rng(5)
    drawn = torch.where(torch.from_numpy(rng.integers(0, 3, size=(Bn, N)) == 0).to(dev), (applied - 3.0).clamp(min=0.0), applied).contiguous()
    present = ((cur.s_len[:, 0] > 0) & (cur.s_off[:, 0] == 0)).to(torch.int32)
    fresh = (torch.from_numpy((rng.integers(0, 8, size=(Bn, N)) == 0).astype(np.int32)).to(dev) * present).contiguous()
    est0 = torch.from_numpy(rng.uniform(4.0, 33.0, size=(Bn, N))).to(dev)
    est, ub_out = est0.clone(), torch.empty((Bn, N, Tm), dtype=torch.float64, device=dev)
    eflags = torch.empty(Bn, dtype=torch.int32, device=dev)
    out["estimate_launch_ms"] = median_launch(lambda: handle.estimate_device(cur, fresh, est, ub_out, eflags, pilots=applied, actual=drawn,
                                                                               status=cur.status))
    out["shape"] = [int(Bn), int(N), int(Tm)]
    # per EVSE: s_off, s_len, fresh read (4 B each), est, pilots, actual read and est written (8 B each); lb, ub read and
    # ub_out written (Tm x 8 B each)
    per = 3 * 4 + 4 * 8 + 3 * Tm * 8
    out["estimate_bytes_per_evse"] = per
    out["estimate_gb_per_s"] = Bn * N * per / out["estimate_launch_ms"]["median"] / 1e6
    out["advance_gb_per_s"] = Bn * (5 * N * Tm * 8 + 2 * batch.K * N * 16 + N * 8) / out["advance_launch_ms"]["median"] / 1e6
    out["estimate_capped_at"] = int((ub_out < cur.ub).sum().item())
    out["estimate_flags"] = int(torch.count_nonzero(eflags).item())
    out["present_slots"], out["fresh_slots"] = int(present.sum().item()), int(fresh.sum().item())

    # ---- the closed loop ----------------------------------------------------------------------------------------------
    rng = np.random.default_rng(3)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=30, t_span=10, stay=(8, 13)) for _ in range(args.scenarios)]
    records = [[dict(e, max_rate=32.0, battery=battery(n, e)) for n, e in enumerate(f)] for f in fleets]
    requested = sum(e["requested"] for f in records for e in f)

    def loop(**kw):
        alg = AdaptiveSchedulingAlgorithm(obj, **kw)
        alg.register_interface(iface)
        alg.simulate_batch(records, 2)   # warm-up: handle, allocator
        table = FleetTable(records, infra, iface, obj, args.steps)
        alg.simulate_batch(table, args.steps)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = alg.simulate_batch(table, args.steps)
            runs.append(time.perf_counter() - t0)
        return res, {"simulate_batch_s": {"median": statistics.median(runs), "runs": runs},
                     "delivered_fraction": float(sum(d.sum() for d in res.delivered) / requested),
                     "offered_not_drawn_amp_periods": float((res.pilots - res.actual).sum()), "iterations": int(res.iters.sum()),
                     "flags": int(np.count_nonzero(res.flags)), "not_solved": int((~np.isin(res.status, (1, 5))).sum())}

    _, out["closed_loop_without_estimator"] = loop()
    res, out["closed_loop_with_estimator"] = loop(estimate_max_rate=True, max_rate_estimator=SimpleRampdown())
    out["closed_loop_with_estimator"].update(estimate_flags=int(np.count_nonzero(res.estimate_flags)),
                                             finite_estimates_below_32=int((res.estimates < 32.0).sum()))
    out["closed_loop_shape"] = {"scenarios": args.scenarios, "evs": 30, "steps": args.steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
