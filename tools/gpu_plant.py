"""Time the plant launch (acnqp_plant_device) at 16,384 x 54 beside the advance launch (acnqp_advance_device) of the same
batch at Tm = 12, and a closed-loop ``simulate_batch`` of 256 scenarios x 30 EVs x 24 steps with a battery per EV against the
same loop without, all in one process.

    python tools/gpu_plant.py [--batch 16384] [--scenarios 256] [--steps 24] [--out profiles/plant_timing.json]
    python tools/gpu_plant.py --loop-only --out <file>     # the loop without batteries alone: what runs on the commit before

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


def battery(n, ev):
    """a third of the EVs two-stage and past the knee, a third short of room, a third ample"""
    if n % 3 == 0:
        cap = 2.0 * ev["requested"] / 0.15
        return dict(capacity=cap, init_charge=0.85 * cap, max_power=7.0, transition_soc=0.8)
    if n % 3 == 1:
        return dict(capacity=10.0, init_charge=10.0 - 0.6 * ev["requested"], max_power=7.0, transition_soc=0.9)
    return dict(capacity=100.0, init_charge=0.0, max_power=7.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--scenarios", type=int, default=256)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plant_timing.json"))
    args = ap.parse_args()

    import torch

    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.rollout import FleetTable
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

    if not args.loop_only:
        from adacharge_amd.adaptive_charging_optimization import _site_handle
        from adacharge_amd.backend import AdvancePlan, DeviceBatch, PlantPlan, default_options
        from adacharge_amd.builder import build_batch_from_table, objective_terms

        # ---- one launch of either kernel on the same solved batch ------------------------------------------------------
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
        k = 208.0 * 5 / 1e3 / 60
        rng = np.random.default_rng(5)
        R = 4096                                                              # a table of 4,096 batteries, a third of them two-stage
        capacity, soc = rng.uniform(20.0, 100.0, R), rng.uniform(0.1, 0.97, R)
        knee = np.where(np.arange(R) % 3 == 0, 0.2 * capacity / k, 0.0)
        amps = np.full(R, 7000.0 / 208.0)
        table = dict(t_room=(1 - soc) * capacity / k, t_amps=amps, t_knee=knee, t_slope=np.where(knee > 0, amps / np.where(knee > 0, knee, 1.0), 0.0))
        pplan = PlantPlan(plug=np.full((Bn, N), -1, np.int32), **table).to_device(dev)
        bat = torch.from_numpy(rng.integers(-1, R, size=(Bn, N)).astype(np.int32)).to(dev)
        room0 = torch.from_numpy(table["t_room"]).to(dev)[bat.clamp(min=0).long()].contiguous()
        room, actual = room0.clone(), torch.empty((Bn, N), dtype=torch.float64, device=dev)
        pflags = torch.empty(Bn, dtype=torch.int32, device=dev)
        out["plant_launch_ms"] = median_launch(lambda: handle.plant_device(cur, pplan, applied, bat, room, actual, pflags, status=cur.status))
        out["shape"] = [int(Bn), int(N), int(Tm)]
        # per EVSE: s_off, s_len, plug, bat read (4 B each), pilots and room read (8 B each); bat, room, actual written
        moved = Bn * N * (4 * 4 + 2 * 8 + 4 + 2 * 8)
        out["plant_bytes_per_evse"] = 4 * 4 + 2 * 8 + 4 + 2 * 8
        out["plant_gb_per_s"] = moved / out["plant_launch_ms"]["median"] / 1e6
        out["advance_gb_per_s"] = Bn * (5 * N * Tm * 8 + 2 * batch.K * N * 16 + N * 8) / out["advance_launch_ms"]["median"] / 1e6
        out["plant_drew_less_at"] = int((actual < applied).sum().item())

    # ---- the closed loop ----------------------------------------------------------------------------------------------
    rng = np.random.default_rng(3)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=30, t_span=10, stay=(8, 13)) for _ in range(args.scenarios)]
    alg = AdaptiveSchedulingAlgorithm(obj)
    alg.register_interface(iface)

    def loop(records):
        alg.simulate_batch(records, 2)   # warm-up: handle, allocator
        table = FleetTable(records, infra, iface, obj, args.steps)
        alg.simulate_batch(table, args.steps)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = alg.simulate_batch(table, args.steps)
            runs.append(time.perf_counter() - t0)
        requested = sum(e["requested"] for f in records for e in f)
        return res, {"simulate_batch_s": {"median": statistics.median(runs), "runs": runs},
                     "delivered_fraction": float(sum(d.sum() for d in res.delivered) / requested),
                     "flags": int(np.count_nonzero(res.flags)), "not_solved": int((~np.isin(res.status, (1, 5))).sum())}

    plain = [[dict(e, max_rate=32.0) for e in f] for f in fleets]
    _, out["closed_loop_without_batteries"] = loop(plain)
    if not args.loop_only:
        res, out["closed_loop_with_batteries"] = loop([[dict(e, battery=battery(n, e)) for n, e in enumerate(f)] for f in plain])
        out["closed_loop_with_batteries"].update(plant_flags=int(np.count_nonzero(res.plant_flags)),
                                                 drew_less_at=int((res.actual < res.pilots).sum()))
    out["closed_loop_shape"] = {"scenarios": args.scenarios, "evs": 30, "steps": args.steps}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
