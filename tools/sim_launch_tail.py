"""How long the headline step's launches must take, from the CPU twin's iteration counts alone (no GPU): a SIMULATION.

    python tools/sim_launch_tail.py [--rank R] [--site K] [--us-per-iteration 3.67] [--threads 8] [--cap-iterations 808]

The bench's 16,384 problems (caltech54, horizon 12, SOC, the seeds of bench.py for rank R) are solved by the twin
(oracle/admm_port.c; its iteration counts are the wave kernel's), and the counts are list-scheduled on the chip's 1,024
wave slots (256 CUs x one workgroup of four waves; a wave takes the next queue position when it is free) at a fixed time
per wave-iteration (default 3.67 us: 2,202 quad-cycles per problem-iteration, profiles/r06_bench_sq_summary.json, at
2.4 GHz).  Printed, in ms, for each ordering key (the launch order is `largest key first` within a launch):
  even       the solver work spread evenly over the slots: no order can beat it
  lone       one launch of all problems
  pipelined  the chunk plan of a uniform wave call (plan_chunk_caps, acn_qp_pipeline.hpp: 2,048 / 4,096 / 8,192 / 2,048),
             each chunk a launch of its own in call order; a CU passes to the next launch when the slowest of its four
             waves is done (copies, the polish and the launch gaps are not modelled)
Keys, five measures of DEMAND: the session count (order_keys_kernel's key under ACNQP_ORDER_KEY=sessions), sum of s_len,
sum of ub, deliverable energy (sum of s_cap), natural order; four measures of CONGESTION, all of the greedy schedule of
tests/order_key_spec.py (every session at its upper bound until its cap is used up) set against the site rows:
  overload_cells                    C, the (row, period) cells whose load exceeds the limit
  overload_key                      8 min(C, 127) + min(7, sessions / 8): what order_keys_kernel computes
  max_ratio_q128                    the largest load / limit of any cell, in steps of 1 / 128
  overload_periods_x64_plus_sessions  periods with an overloaded cell, times 64, plus the session count
and -- as the bound for any key -- the true iteration counts.  Every key also reports its makespans in wave-iterations.
--site K: instead of the headline workload, the 1,024 demand scenarios of site K of bench.py's configs[3] legs
(cfg3_site in bench.py), one launch on 512 and on 1,024 slots; `lone_iterations_by_slots` per key.

The step in TIME (`timed`, printed with --link-gbs; the launch-order key the library ships, overload_key):
  --link-gbs G   chunk c's launch cannot start before its inputs have landed: 21.65 KB per problem (bench shape: lb, ub, q
                 and the small arrays) over a host link of G GB/s, the chunks' inputs one after the other, plus 60 us for
                 the order kernels and the launch; behind each chunk the copy of its schedules (5,184 B per problem, the
                 link's other direction, one copy at a time) -- the step ends with the last of them
  --direct       no result copy behind a chunk (the kernel stores the schedules into the caller's pinned arrays)
  --plan a,b,c   explicit chunk sizes, the rest in a last chunk (like ACNQP_PLAN); several plans separated by `/`
`--plan` without --link-gbs replaces the chunk plan of `pipelined`."""
import argparse
import heapq
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVES, PER_WG = 1024, 4


def lone(iters, order, slots=WAVES):
    """makespan (iterations) of one launch: every wave slot takes the next position of the queue when it is free"""
    free = [0] * slots
    heapq.heapify(free)
    end = 0
    for b in order:
        t = heapq.heappop(free) + int(iters[b])
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def pipelined(iters, chunks):
    """makespan of consecutive launches: workgroup slot w (four waves) starts launch c when ITS launch c - 1 workgroup has
    retired, i.e. when the slowest of its four waves found the queue empty; within a launch the waves share one queue"""
    wg_free = np.zeros(WAVES // PER_WG, dtype=np.int64)
    for order in chunks:
        heap = [(int(wg_free[w // PER_WG]), w) for w in range(WAVES)]
        heapq.heapify(heap)
        last = wg_free.copy()
        for b in order:
            t, w = heapq.heappop(heap)
            t += int(iters[b])
            last[w // PER_WG] = max(last[w // PER_WG], t)
            heapq.heappush(heap, (t, w))
        wg_free = last
    return int(wg_free.max())


IN_BYTES, OUT_BYTES, LAUNCH_MS = 21650.0, 54 * 12 * 8.0, 0.060   # per problem in, per problem out, order kernels + launch


def timed(iters, chunks, ms_per_iteration, link_gbs, direct):
    """End of the step in ms: `pipelined` in time, with the chunks' arrival times and (not direct) the result copies."""
    per_ms = link_gbs * 1e6   # bytes per ms
    wg_free = np.zeros(WAVES // PER_WG)
    landed, copy_free, end_step = 0.0, 0.0, 0.0
    for order in chunks:
        landed += len(order) * IN_BYTES / per_ms
        ready = landed + LAUNCH_MS
        heap = [(max(float(wg_free[w // PER_WG]), ready), w) for w in range(WAVES)]
        heapq.heapify(heap)
        last = np.maximum(wg_free, ready)
        for b in order:
            t, w = heapq.heappop(heap)
            t += float(iters[b]) * ms_per_iteration
            last[w // PER_WG] = max(last[w // PER_WG], t)
            heapq.heappush(heap, (t, w))
        wg_free = last
        end = float(last.max())
        if not direct:
            copy_free = max(copy_free, end) + len(order) * OUT_BYTES / per_ms
            end = copy_free
        end_step = max(end_step, end)
    return end_step


def plan_of(text, total):
    caps, left, out = [int(v) for v in text.split(",")], total, []
    for cap in caps:
        if left > 0:
            out.append(min(cap, left))
            left -= out[-1]
    if left > 0:
        out.append(left)
    return out


def plan(total):
    c = 8192   # plan_chunk_caps for 16,384 problems: c / 4, c / 2, c, the rest
    caps, left, out = [c // 4, c // 2, c], total, []
    for cap in caps:
        out.append(min(cap, left))
        left -= out[-1]
    if left > 0:
        out.append(left)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--site", type=int, default=None, help="site K of bench.py's configs[3] legs instead of the headline workload")
    ap.add_argument("--us-per-iteration", type=float, default=2202 * 4 / 2.4e3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--cap-iterations", type=int, default=808,
                    help="the device hands a problem to the polish after 800 iterations (808 is the most it reports on this workload); the twin iterates on")
    ap.add_argument("--link-gbs", type=float, default=None, help="host link in GB/s: print the step in time (`timed`)")
    ap.add_argument("--direct", action="store_true", help="with --link-gbs: no result copy behind a chunk")
    ap.add_argument("--plan", default=None, help="explicit chunk sizes a,b,c (the rest in a last chunk); several plans separated by /")
    ap.add_argument("--save-iterations", default=None, help="keep the twin's iteration counts and keys in this .npz (and reuse them)")
    args = ap.parse_args()

    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch, make_site
    from oracle import admm_port

    from tests import order_key_spec as spec

    DEMAND = ("sessions", "sum_s_len", "sum_ub", "energy")
    CONGESTION = ("overload_cells", "overload_key", "max_ratio_q128", "overload_periods_x64_plus_sessions")

    def keys_of(batch):
        s_len = np.asarray(batch.s_len).reshape(batch.B, -1)
        ratios, C, key = spec.describe(batch)
        over = ratios > spec.OVERLOAD
        finite = np.where(np.isfinite(ratios), ratios, 0.0).reshape(batch.B, -1)
        worst = finite.max(axis=1) if finite.shape[1] else np.zeros(batch.B)
        return {"sessions": (s_len > 0).sum(axis=1), "sum_s_len": s_len.sum(axis=1),
                "sum_ub": np.asarray(batch.ub).reshape(batch.B, -1).sum(axis=1),
                "energy": np.asarray(batch.s_cap).reshape(batch.B, -1).sum(axis=1),
                "overload_cells": C, "overload_key": key.astype(np.int64),
                "max_ratio_q128": np.minimum(1023, np.floor(worst * 128)).astype(np.int64),
                "overload_periods_x64_plus_sessions": over.any(axis=1).sum(axis=1) * 64 + (s_len > 0).sum(axis=1)}

    if args.site is not None:
        # bench.py, cfg3_site(k): one snapshot of the site, 1,024 lognormal demand scenarios
        from adacharge_amd.builder import scenario_batch

        infra = sites.eight_sites()[args.site]
        iface = Interface({"infrastructure_info": infra, "period": 5})
        rng = np.random.default_rng(500 + args.site)
        qc_es = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
        base = build_batch([sites.random_sessions(infra, 12, rng)], infra, iface, qc_es, "SOC")
        batch = scenario_batch(base, rng.lognormal(0.0, 0.25, size=(1024, base.K, base.N)))
        iters = np.minimum(admm_port.solve_batch(batch, threads=args.threads, accel_mem=5)["iters"].astype(np.int64), args.cap_iterations)
        keys = keys_of(batch)
        keys["natural"] = np.zeros(iters.size)
        keys["true_iterations"] = iters
        out = {"simulation": "list schedule of the CPU twin's iteration counts; nothing here was measured on a GPU",
               "site": args.site, "evse": int(batch.N), "site_rows": int(batch.site.Mg), "problems": int(iters.size),
               "mean_iterations": float(iters.mean()), "max_iterations": int(iters.max()),
               "no_overloaded_cell": int((keys["overload_cells"] == 0).sum()),
               "even_iterations_by_slots": {str(s_): float(iters.sum() / s_) for s_ in (512, 1024)}, "keys": {}}
        for name, key in keys.items():
            order = np.argsort(-key, kind="stable")
            out["keys"][name] = {"lone_iterations_by_slots": {str(s_): lone(iters, order, s_) for s_ in (512, 1024)}}
        print(json.dumps(out, indent=1))
        raise SystemExit(0)

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    objective = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    site = make_site(infra, "SOC")
    if args.save_iterations and os.path.exists(args.save_iterations):
        with np.load(args.save_iterations) as z:
            raw_iters, keys = z["raw_iters"], {k: z[k] for k in DEMAND + CONGESTION}
    else:
        iters, keys = [], {k: [] for k in DEMAND + CONGESTION}
        for g in range(args.batches):
            sn = sites.snapshot_batch(infra, 12, 256, seed=20240 + 7919 * args.rank + 104729 * g)
            batch = build_batch(sn, infra, iface, objective, "SOC", site=site)
            iters.append(admm_port.solve_batch(batch, threads=args.threads, accel_mem=5)["iters"])
            for k, v in keys_of(batch).items():
                keys[k].append(v)
        raw_iters = np.concatenate(iters).astype(np.int64)
        keys = {k: np.concatenate(v) for k, v in keys.items()}
        if args.save_iterations:
            np.savez_compressed(args.save_iterations, raw_iters=raw_iters, **keys)
    iters = np.minimum(raw_iters, args.cap_iterations)
    keys["natural"] = np.zeros(iters.size)
    keys["true_iterations"] = iters
    total = iters.size
    ms = args.us_per_iteration * 1e-3
    sizes = plan_of(args.plan.split("/")[0], total) if args.plan else plan(total)
    bounds = np.r_[0, np.cumsum(sizes)]
    by_sessions = np.argsort(-keys["sessions"], kind="stable")
    out = {"simulation": "list schedule of the CPU twin's iteration counts; nothing here was measured on a GPU",
           "rank": args.rank, "problems": int(total), "mean_iterations": float(iters.mean()), "max_iterations": int(iters.max()),
           "us_per_iteration": args.us_per_iteration, "wave_slots": WAVES, "chunk_plan": [int(s) for s in sizes],
           "even_ms": float(iters.sum() / WAVES * ms),
           "at_least_400_iterations": int((iters >= 400).sum()),
           "at_least_400_in_last_6384_of_session_order": int((iters[by_sessions[-6384:]] >= 400).sum()),
           "no_overloaded_cell": int((keys["overload_cells"] == 0).sum()),
           "first_check_20_iterations": int((raw_iters == 20).sum()),
           "no_overloaded_cell_xor_20_iterations": int(((keys["overload_cells"] == 0) != (raw_iters == 20)).sum()),
           "keys": {}}
    for name, key in keys.items():
        order = np.argsort(-key, kind="stable")
        chunks = [lo + np.argsort(-key[lo:hi], kind="stable") for lo, hi in zip(bounds[:-1], bounds[1:])]
        li, pi = lone(iters, order), pipelined(iters, chunks)
        l, p = li * ms, pi * ms
        out["keys"][name] = {"lone_ms": round(l, 2), "pipelined_ms": round(p, 2), "lone_over_even": round(l / out["even_ms"] - 1, 3),
                             "pipelined_over_even": round(p / out["even_ms"] - 1, 3), "lone_iterations": li, "pipelined_iterations": pi}
    if args.link_gbs:
        key = keys["overload_key"]
        out["timed"] = {"link_gbs": args.link_gbs, "direct": bool(args.direct), "key": "overload_key", "end_of_step_ms": {}}
        for text in (args.plan.split("/") if args.plan else [",".join(str(v) for v in sizes)]):
            b_ = np.r_[0, np.cumsum(plan_of(text, total))]
            chunks = [lo + np.argsort(-key[lo:hi], kind="stable") for lo, hi in zip(b_[:-1], b_[1:])]
            out["timed"]["end_of_step_ms"]["/".join(str(int(hi - lo)) for lo, hi in zip(b_[:-1], b_[1:]))] = round(timed(iters, chunks, ms, args.link_gbs, args.direct), 3)
    print(json.dumps(out, indent=1))
