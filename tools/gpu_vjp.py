"""Time one launch of the adjoint KKT kernel (acnqp_vjp_device, adacharge_amd/csrc/acn_qp_vjp.hpp) at the headline shape,
16,384 x 54 x 12, against the solve launch of the same batch, in one process.

    python tools/gpu_vjp.py [--batch 16384] [--horizon 12] [--out profiles/vjp_timing.json]
    python tools/gpu_vjp.py --long [--out profiles/vjp_long_timing.json]

``--long``: the long-horizon kernel (adacharge_amd/csrc/acn_qp_vjp_long.hpp, ``solver_options={"vjp_long": True}``) at
256 x 54 x 144 and at 16 x 54 x 288, each beside its batch's solve launch, into one file.

The kernel time is the median of 5 launches between HIP events (one warm-up launch first); the solve time is the sum of
the HIP-event durations of the call's launches (``BatchResult.kernel_ms``).  Nothing is asserted about any time.  The
gradient is taken at the solver's own answer (default options), with dL/dx = 1 on every rate.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


LONG_SHAPES = ((256, 144), (16, 288))   # (batch, horizon) of --long


def measure(batch_size, horizon, solver_options=None):
    """one shape: the solve, then the timed adjoint launches at its answer"""
    import torch

    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd import session_table as st
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import DeviceBatch

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    table = st.enforce_pilot_limit(sites.snapshot_table(infra, horizon, batch_size), infra)
    opt = AdaptiveChargingOptimization([ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)], iface, "SOC",
                                       solver_options=solver_options)
    res, _ = opt.solve_table(table, infra)
    handle, batch = res.handle, opt.last_batch
    dev = DeviceBatch(batch, torch.device("cuda", handle.device), want_y=True)
    dev.x.copy_(torch.from_numpy(res.x))
    dev.y.copy_(torch.from_numpy(res.y))
    dev.status.copy_(torch.from_numpy(res.status))
    B, N, Tm, K = dev.B, dev.N, dev.Tm, dev.K
    nrow = batch.site.M + int(bool(batch.site.has_peak))
    f8 = dict(dtype=torch.float64, device=dev.x.device)
    gx = torch.ones((B, N, Tm), **f8)
    gq, glb, gub = (torch.empty((B, N, Tm), **f8) for _ in range(3))
    gcap, grow, r = torch.empty((B, K, N), **f8), torch.empty((B, nrow, Tm), **f8), torch.empty((B, 2), **f8)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev.x.device)

    def launch(bounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        handle.vjp_device(dev, gx, gq, gcap, grow, info, r, glb=glb if bounds else None, gub=gub if bounds else None,
                          options=opt._last_options, stream=torch.cuda.current_stream().cuda_stream)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    launch(True)
    full = [launch(True) for _ in range(5)]
    lean = [launch(False) for _ in range(5)]
    inf, rr = info.cpu().numpy(), r.cpu().numpy()
    done = inf[:, 0] == 0
    return {
        "shape": [int(B), int(N), int(Tm)],
        "device": torch.cuda.get_device_name(dev.x.device),
        "vjp_launch_ms": {"median": statistics.median(full), "runs": full},
        "vjp_without_bounds_launch_ms": {"median": statistics.median(lean), "runs": lean},
        "solve_launch_ms": float(res.kernel_ms),
        "solved": int(np.isin(res.status, (1, 5)).sum()),
        "verdicts": {str(v): int((inf[:, 0] == v).sum()) for v in range(4)},
        "schur_rows": {"max": int(inf[done, 1].max()), "mean": float(inf[done, 1].mean())},
        "problems_with_weak_members": int((inf[done, 2] > 0).sum()),
        "free_variables_mean": float(inf[done, 3].mean()),
        "solve_residual_max": float(rr[done, 0].max()),
        "stationarity": {"median": float(np.median(rr[done, 1])), "max": float(rr[done, 1].max())},
    }


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--long", action="store_true", help="the long-horizon kernel at 256 x 54 x 144 and 16 x 54 x 288")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.long:
        args.out = args.out or os.path.join(root, "profiles", "vjp_long_timing.json")
        out = {"solver_options": {"vjp_long": True}, "launches": [measure(b, t, {"vjp_long": True}) for b, t in LONG_SHAPES]}
    else:
        args.out = args.out or os.path.join(root, "profiles", "vjp_timing.json")
        out = measure(args.batch, args.horizon)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
