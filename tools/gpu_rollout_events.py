"""Time a closed-loop ``simulate_batch`` that solves every scenario at every period (``resolve="every_step"``) against one
that re-solves on events only (``resolve="events"``, max_recompute None and 4), all in one process on one build: caltech54,
256 scenarios of ``closed_loop_fleet(n_evs=5, t_span=40, stay=(8, 13))``, 48 steps at t_max = 12.

    python tools/gpu_rollout_events.py [--scenarios 256] [--steps 48] [--out profiles/rollout_events.json]

Printed: the share of (step, scenario) pairs solved, the solver launches per run (acnqp_launch_count), the three times --
each the median of five end-to-end calls after one untimed warm-up call, with min and max -- the sum of the solver launches'
own durations over one more run (acnqp_kernel_times) beside what that run's host-side sum of delivered energy takes (it is
part of every call, whatever was solved), and the time of one select and
one hold launch between stream events at the run's mean step (B scenarios, the mean number of them resolving).  Nothing is
asserted about any time: a small launch lasts as long as its slowest problem, so time need not fall in proportion.
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
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_events.json"))
    args = ap.parse_args()

    import torch

    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.adaptive_charging_optimization import _site_handle
    from adacharge_amd.backend import DeviceBatch
    from adacharge_amd.rollout import FleetTable
    from tests import helpers

    B, steps, Tm = args.scenarios, args.steps, 12
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    rng = np.random.default_rng(3)
    fleets = [[dict(e, max_rate=32.0) for e in helpers.closed_loop_fleet(infra, rng, n_evs=5, t_span=40, stay=(8, 13))] for _ in range(B)]
    table = FleetTable(fleets, infra, iface, obj, steps, t_max=Tm)
    dev = torch.device("cuda", 0)
    site, handle = _site_handle(infra, "SOC", False, 0)
    launches = lambda: int(handle._lib.acnqp_launch_count(handle._h))
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"scenarios": B, "evs": 5, "steps": steps, "t_max": Tm}, "runs": {}}

    for name, resolve, mr in (("every_step", "every_step", None), ("events", "events", None), ("events_max_recompute_4", "events", 4)):
        alg = AdaptiveSchedulingAlgorithm(obj, max_recompute=mr)
        alg.register_interface(iface)
        alg.simulate_batch(table, steps, resolve=resolve)   # warm-up: handle, allocator, plan upload paths
        n0 = launches()
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            res = alg.simulate_batch(table, steps, resolve=resolve)
            times.append(time.perf_counter() - t0)
        per_run = (launches() - n0) / 5
        handle.kernel_times()                                # forget earlier launches; one more run, for the solver launches' own time
        t0 = time.perf_counter()
        alg.simulate_batch(table, steps, resolve=resolve)
        t1 = time.perf_counter()
        table.delivered(res.pilots)
        t2 = time.perf_counter()
        ms = handle.kernel_times()
        mask = np.ones((steps, B), bool) if resolve == "every_step" else table.resolve_rows(mr)
        out["runs"][name] = {"share_solved": float(mask.mean()), "steps_nobody_resolves": int((mask.sum(axis=1) == 0).sum()),
                             "steps_everybody_resolves": int(mask.all(axis=1).sum()), "solver_launches_per_run": per_run,
                             "simulate_batch_s": {"median": statistics.median(times), "min": min(times), "max": max(times)},
                             "solver_kernel_ms_per_run": {"sum": float(sum(ms)), "launches_timed": len(ms)},
                             "of_one_run_s": {"simulate_batch": t1 - t0, "its_host_sum_of_delivered_energy": t2 - t1},
                             "iterations": int(res.iters.sum()), "not_solved": int((~np.isin(res.status, (1, 5))).sum()),
                             "flags": int(np.count_nonzero(res.flags))}

    # ---- one select and one hold launch at the run's mean step --------------------------------------------------------------
    m = max(1, int(round(table.resolve_rows(None).sum(axis=1).mean())))
    idx = np.sort(rng.choice(B, size=m, replace=False)).astype(np.int32)
    pos = np.full(B, -1, np.int32)
    pos[idx] = np.arange(m, dtype=np.int32)
    cur, dense = DeviceBatch.empty(site, B, Tm, 1, dev), DeviceBatch.empty(site, B, Tm, 1, dev)
    didx, dpos = torch.from_numpy(idx).to(dev), torch.from_numpy(pos).to(dev)
    held = torch.zeros((B, site.N, Tm), dtype=torch.float64, device=dev)
    prev = torch.ones(B, dtype=torch.int32, device=dev)
    flags, solved = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    part = dense.head(m)

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
        return {"median": statistics.median(runs), "min": min(runs), "max": max(runs)}

    stream = torch.cuda.current_stream(dev).cuda_stream
    out["select_launch_ms"] = median_launch(lambda: handle.select_device(cur, dense, didx, flags, m, stream=stream))
    out["hold_launch_ms"] = median_launch(lambda: handle.hold_device(cur, part, dpos, m, held, prev, solved, flags, stream=stream))
    out["select_hold_shape"] = {"B": B, "m": m}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
