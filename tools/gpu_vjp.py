"""Time one launch of the adjoint KKT kernel (acnqp_vjp_device, adacharge_amd/csrc/acn_qp_vjp.hpp) at the headline shape,
16,384 x 54 x 12, against the solve launch of the same batch, in one process.

    python tools/gpu_vjp.py [--batch 16384] [--horizon 12] [--out profiles/vjp_timing.json]
    python tools/gpu_vjp.py --long [--out profiles/vjp_long_timing.json]
    python tools/gpu_vjp.py --rollout [--out profiles/rollout_vjp_timing.json]

``--long``: the long-horizon kernel (adacharge_amd/csrc/acn_qp_vjp_long.hpp, ``solver_options={"vjp_long": True}``) at
256 x 54 x 144 and at 16 x 54 x 288, each beside its batch's solve launch, into one file.

``--rollout``: the backward sweep through a closed loop (``rollout.rollout_gradients``: per step acnqp_advance_vjp_device and
acnqp_vjp_device) beside its forward rollout (``simulate_batch(..., keep_tape=True)``) at 256 scenarios x caltech54 x t_max 12 x
48 steps, each between HIP events on the current stream, the median of 5 after one warm-up.

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


ROLLOUT_SHAPE = dict(scenarios=256, t_max=12, steps=48, evs=30)


def measure_rollout(scenarios, t_max, steps, evs):
    """the forward rollout with a tape and the backward sweep through it, each the median of 5 between HIP events"""
    import torch

    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, sites, total_energy, tou_energy_cost
    from adacharge_amd.acn import Interface
    from adacharge_amd.rollout import FleetTable, rollout_gradients

    infra = sites.caltech54()
    rng = np.random.default_rng(2024)
    rate = 0.15
    prices = np.where((np.arange(steps + t_max) // 6) % 2 == 0, 0.08, 0.22) + 1e-3 * rng.random(steps + t_max)
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0, "prices": prices})
    k = infra.voltages[0] * 5 / 1e3 / 60
    fleets = []
    for _ in range(scenarios):
        fleet = []
        for n, i in enumerate(rng.choice(infra.num_stations, size=evs, replace=False)):
            arr, dur = int(rng.integers(0, steps - 4)), int(rng.integers(6, t_max + 1))
            fleet.append(dict(station=infra.station_ids[int(i)], arrival=arr, departure=arr + dur, max_rate=32.0,
                              requested=float(rng.uniform(0.3, 0.9) * 32 * dur * k)))
        fleets.append(fleet)
    alg = AdaptiveSchedulingAlgorithm([ObjectiveComponent(total_energy, rate), ObjectiveComponent(equal_share, 1e-5),
                                       ObjectiveComponent(tou_energy_cost)])
    alg.register_interface(iface)
    table = FleetTable(fleets, infra, iface, alg.objective, steps, t_max=t_max)
    w = torch.from_numpy(np.einsum("i,bs->sbi", table.c_weight, table.c_series[:, :steps]).copy()).cuda()   # dL/dpilots of the energy cost

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    forward = lambda: alg.simulate_batch(table, steps, keep_tape=True)
    timed(forward)
    fwd = []
    for _ in range(5):
        ms, res = timed(forward)
        fwd.append(ms)
    timed(lambda: rollout_gradients(res, w))
    bwd = []
    for _ in range(5):
        ms, g = timed(lambda: rollout_gradients(res, w))
        bwd.append(ms)
    info = g.info.cpu().numpy()
    return {
        "shape": {"scenarios": scenarios, "evse": int(infra.num_stations), "t_max": t_max, "steps": steps, "evs_per_scenario": evs},
        "device": torch.cuda.get_device_name(0),
        "forward_rollout_ms": {"median": statistics.median(fwd), "runs": fwd},
        "backward_sweep_ms": {"median": statistics.median(bwd), "runs": bwd},
        "launches_of_the_sweep": 2 * steps + 1,
        "solved": int(np.isin(res.status, (1, 5)).sum()), "problems": int(res.status.size),
        "verdicts": {str(v): int((info[:, :, 0] == v).sum()) for v in range(4)},
        "price_gradient_abs_max": float(g.prices.abs().max().item()),
    }


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--long", action="store_true", help="the long-horizon kernel at 256 x 54 x 144 and 16 x 54 x 288")
    ap.add_argument("--rollout", action="store_true", help="a backward sweep through a 256 x caltech54 x t_max 12 x 48-step rollout")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rollout:
        args.out = args.out or os.path.join(root, "profiles", "rollout_vjp_timing.json")
        out = measure_rollout(**ROLLOUT_SHAPE)
    elif args.long:
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
