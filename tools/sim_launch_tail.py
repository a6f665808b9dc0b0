"""How long the headline step's launches must take, from the CPU twin's iteration counts alone (no GPU): a SIMULATION.

    python tools/sim_launch_tail.py [--rank R] [--us-per-iteration 3.67] [--threads 8] [--cap-iterations 808]

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
Keys: the session count (what order_keys_kernel sorts by), sum of s_len, sum of ub, deliverable energy (sum of s_cap),
natural order, and -- as the bound for any key -- the true iteration counts."""
import argparse
import heapq
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVES, PER_WG = 1024, 4


def lone(iters, order):
    """makespan (iterations) of one launch: every wave slot takes the next position of the queue when it is free"""
    free = [0] * WAVES
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
    ap.add_argument("--us-per-iteration", type=float, default=2202 * 4 / 2.4e3)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--cap-iterations", type=int, default=808,
                    help="the device hands a problem to the polish after 800 iterations (808 is the most it reports on this workload); the twin iterates on")
    args = ap.parse_args()

    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch, make_site
    from oracle import admm_port

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    objective = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    site = make_site(infra, "SOC")
    iters, keys = [], {"sessions": [], "sum_s_len": [], "sum_ub": [], "energy": []}
    for g in range(args.batches):
        sn = sites.snapshot_batch(infra, 12, 256, seed=20240 + 7919 * args.rank + 104729 * g)
        batch = build_batch(sn, infra, iface, objective, "SOC", site=site)
        iters.append(admm_port.solve_batch(batch, threads=args.threads, accel_mem=5)["iters"])
        s_len = np.asarray(batch.s_len).reshape(batch.B, -1)
        keys["sessions"].append((s_len > 0).sum(axis=1))
        keys["sum_s_len"].append(s_len.sum(axis=1))
        keys["sum_ub"].append(np.asarray(batch.ub).reshape(batch.B, -1).sum(axis=1))
        keys["energy"].append(np.asarray(batch.s_cap).reshape(batch.B, -1).sum(axis=1))
    iters = np.minimum(np.concatenate(iters).astype(np.int64), args.cap_iterations)
    keys = {k: np.concatenate(v) for k, v in keys.items()}
    keys["natural"] = np.zeros(iters.size)
    keys["true_iterations"] = iters
    total = iters.size
    ms = args.us_per_iteration * 1e-3
    sizes = plan(total)
    bounds = np.r_[0, np.cumsum(sizes)]
    by_sessions = np.argsort(-keys["sessions"], kind="stable")
    out = {"simulation": "list schedule of the CPU twin's iteration counts; nothing here was measured on a GPU",
           "rank": args.rank, "problems": int(total), "mean_iterations": float(iters.mean()), "max_iterations": int(iters.max()),
           "us_per_iteration": args.us_per_iteration, "wave_slots": WAVES, "chunk_plan": [int(s) for s in sizes],
           "even_ms": float(iters.sum() / WAVES * ms),
           "at_least_400_iterations": int((iters >= 400).sum()),
           "at_least_400_in_last_6384_of_session_order": int((iters[by_sessions[-6384:]] >= 400).sum()),
           "keys": {}}
    for name, key in keys.items():
        order = np.argsort(-key, kind="stable")
        chunks = [lo + np.argsort(-key[lo:hi], kind="stable") for lo, hi in zip(bounds[:-1], bounds[1:])]
        l, p = lone(iters, order) * ms, pipelined(iters, chunks) * ms
        out["keys"][name] = {"lone_ms": round(l, 2), "pipelined_ms": round(p, 2), "lone_over_even": round(l / out["even_ms"] - 1, 3),
                             "pipelined_over_even": round(p / out["even_ms"] - 1, 3)}
    print(json.dumps(out, indent=1))
