"""The long-horizon polish (adacharge_amd/csrc/acn_qp_polish_long.hpp) against the same build with the switch off: lone
device-resident launches under default options, the two settings interleaved, medians of N launches each.

    python3 tools/gpu_polish_long.py [--launches 5] [--out profiles/polish_long.json] [leg ...]

Legs: stress_b256, stress_b2048 (the reference's stress shape, 54 EVSE x 144 periods: bench.other_workloads), offline_day
(sites.offline_day at 288 periods on the Caltech site, 16 days; at most four sessions per EVSE so that the shape stays on the
long-horizon kernel).  Per leg and setting: the lone launch time (acnqp_kernel_times), iters mean and max, statuses, and with
the switch on the problems handed over and solved, the Newton rounds, workgroup-microseconds per round (the kernel's phase
clock) and the slab bytes of a workgroup."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from adacharge_amd.backend import DeviceBatch, SiteHandle, default_options


def offline_days(n_days=16, horizon=288):
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    days = []
    for d in range(n_days):
        sl = sites.offline_day(infra, np.random.default_rng(2880 + d), horizon=horizon)
        seen, keep = {}, []
        for s in sl:   # the first four sessions of an EVSE: one slot each
            seen[s.station_id] = seen.get(s.station_id, 0) + 1
            if seen[s.station_id] <= 4:
                keep.append(s)
        days.append(keep)
    return build_batch(days, infra, iface, obj, "SOC")


def slab_bytes(site, t_max, k):
    """PolishLongLayout::slab_total of acn_qp_polslab.hpp, restated: bytes of one workgroup's slab"""
    N, Mg, nrow = int(site.N), int(site.Mg), int(site.M) + int(bool(site.has_peak))
    rows, sess = Mg * t_max, ((N * k + 7) // 8) * 8
    blk = Mg * (Mg + 1) // 2
    lds = Mg * N + 4 * blk + 8 * Mg + 64 * Mg + 3 * sess + 16 + (2 * (t_max + 1) + 4 * sess + 4 * N + 128 + 8 + 1) // 2
    cap = sess * (sess + 1) // 2
    d = 8 * N * t_max + 2 * Mg * t_max + nrow * t_max + 5 * rows + t_max * blk + (0 if (lds + cap) * 8 <= 152 * 1024 else cap)
    d += (3 * rows + 1) // 2 + (2 * N * t_max + nrow * t_max + 7) // 8
    return 8 * ((d + 1) & ~1)


def measure(batch, launches):
    dev = torch.device("cuda", 0)
    handles = {"off": SiteHandle(batch.site, 0), "on": SiteHandle(batch.site, 0, polish_long=True)}
    dbs = {k: DeviceBatch(batch, dev) for k in handles}
    o = default_options()
    out = {k: {"ms": []} for k in handles}
    stream = torch.cuda.current_stream().cuda_stream
    for k, h in handles.items():   # warm-up: code objects, workspaces
        h.solve_device(dbs[k], o, stream=stream)
        torch.cuda.synchronize()
        h.kernel_times()
    s0 = handles["on"].polish_stats()
    for _ in range(launches):      # interleaved
        for k, h in handles.items():
            h.solve_device(dbs[k], o, stream=stream)
            torch.cuda.synchronize()
            out[k]["ms"] += h.kernel_times()
    s1 = handles["on"].polish_stats()
    for k, h in handles.items():
        it, st = dbs[k].iters.cpu().numpy(), dbs[k].status.cpu().numpy()
        fam, pol = h.route(batch.Tm, batch.K, batch.B)
        ms = sorted(out[k]["ms"])
        out[k] = {"family": fam, "polish": int(pol), "ms_median": round(float(np.median(ms)), 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                  "launches": len(ms), "iters_mean": round(float(it.mean()), 1), "iters_max": int(it.max()),
                  "status": {str(int(v)): int(c) for v, c in zip(*np.unique(st, return_counts=True))}}
    x_off, x_on = dbs["off"].x.cpu().numpy(), dbs["on"].x.cpu().numpy()
    per = {c: (s1[c] - s0[c]) / launches for c in ("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt", "rounds")}
    us = sum(s1["phase_us"]) - sum(s0["phase_us"])
    out["on"]["per_launch"] = per
    out["on"]["workgroup_us_per_round"] = round(us / max(1, s1["rounds"] - s0["rounds"]), 1)
    out["on"]["phase_us_share"] = [round((a - b) / max(1, us), 3) for a, b in zip(s1["phase_us"], s0["phase_us"])]
    out["on"]["slab_bytes_per_workgroup"] = slab_bytes(batch.site, batch.Tm, batch.K)
    out["max_abs_diff_on_vs_off_A"] = float(np.abs(x_on - x_off).max())
    for h in handles.values():
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    wl = bench.other_workloads()
    legs = {"stress_b256": lambda: wl["stress_caltech54_T144_b256"]()[0], "stress_b2048": lambda: wl["stress_caltech54_T144_b2048"]()[0],
            "offline_day": offline_days}
    res = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "options": "acnqp_default_options", "legs": {}}
    for name in a.legs or list(legs):
        batch = legs[name]()
        r = measure(batch, a.launches)
        r["shape"] = {"B": int(batch.B), "N": int(batch.N), "t_max": int(batch.Tm), "K": int(batch.K), "Mg": int(batch.site.Mg)}
        res["legs"][name] = r
        print(json.dumps({name: r}), flush=True)
        if a.out:   # (after every leg: a run that is cut short keeps what it has)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
