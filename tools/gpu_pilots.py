"""Time the REALLOCATE launch of the pilot-signal kernel (acnqp_pilots_device) at the headline shape, 16,384 x 54 x 12,
against the solve launch of the same batch and the host's ``diff_based_reallocation_batch``, all in one process.

    python tools/gpu_pilots.py [--batch 16384] [--out profiles/pilots_timing.json]

The kernel time is the median of 5 launches between HIP events (one warm-up launch first); the solve time is the sum
of the HIP-event durations of the call's launches (``BatchResult.kernel_ms``); the host time is one wall-clock run.
Nothing is asserted about any time; the bits are compared with the host's on the way.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pilots_timing.json"))
    args = ap.parse_args()

    import torch

    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, postprocessing as pp, quick_charge, sites
    from adacharge_amd import session_table as st
    from adacharge_amd.acn import Interface

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    table = st.enforce_pilot_limit(sites.snapshot_table(infra, args.horizon, args.batch), infra)
    opt = AdaptiveChargingOptimization([ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)], iface, "SOC")
    res, _ = opt.solve_table(table, infra, keep_on_device=True)
    handle, x_dev = res.handle, res.x_dev
    dev = x_dev.device
    B, N, Tm = x_dev.shape
    plan = pp.pilot_plan_arrays(table, infra, iface, "reallocate", batch=B, t_max=Tm).to_device(dev)
    pilots = torch.empty_like(x_dev)
    first = torch.empty((B, N), dtype=torch.float64, device=dev)
    visits = torch.empty(B, dtype=torch.int32, device=dev)

    def launch(only_first):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        handle.pilots_device(plan, x_dev, pilots=None if only_first else pilots, first=first, visits=visits)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    launch(False)
    full = [launch(False) for _ in range(5)]
    head = [launch(True) for _ in range(5)]
    t0 = time.perf_counter()
    want = pp.diff_based_reallocation_batch(res.x, table, infra, iface)
    host_s = time.perf_counter() - t0
    got, vis = pilots.cpu().numpy(), visits.cpu().numpy()
    differ = int((got != want).any(axis=(1, 2)).sum())
    out = {
        "shape": [int(B), int(N), int(Tm)],
        "device": torch.cuda.get_device_name(dev),
        "reallocate_launch_ms": {"median": statistics.median(full), "runs": full},
        "reallocate_first_period_only_launch_ms": {"median": statistics.median(head), "runs": head},
        "solve_launch_ms": float(res.kernel_ms),
        "host_diff_based_reallocation_batch_ms": host_s * 1e3,
        "visits": {"max": int(vis.max()), "mean": float(vis.mean()), "stopped_at_bound": int((vis < 0).sum())},
        "snapshots_where_host_and_device_differ": differ,
        "solved": int(np.isin(res.status, (1, 5)).sum()),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
