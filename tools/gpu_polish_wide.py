"""The wide-site polish (adacharge_amd/csrc/acn_qp_polish_wide.hpp) against the same build with the switch off, measured, not
gated.  Writes profiles/polish_wide.json.

    python3 tools/gpu_polish_wide.py [--out profiles/polish_wide.json] [--launches 5] [leg ...]

Every leg runs in a child process of its own under a time limit, and the first leg that fails or runs out of time ends the
run (what the earlier legs measured is kept).  Legs:
  soak          the instance of tools/gpu_soak.py 512 8, case 18 (synth512 x 48, SOC, energy equalities; its seed), under that
                tool's options (max_iter 30,000), switch off and on: statuses, worst site-row violation, iters, Newton rounds,
                the polish counters, launch time
  switch_cost   what the switch costs where little or nothing is listed: 2,048 problems of 512 x 48 (SOC, energy equalities,
                8 snapshots x 256 demand scenarios), default options, off and on interleaved, medians of --launches
  round_cost    workgroup-microseconds per Newton round at 512 x 48 from the kernel's phase clock, with the shares of the
                phases (index 2: the capacitance accumulation, 3: its factorisation and the solves): four snapshots of the soak
                class stopped at max_iter 800 with tolerances nothing meets, so that every one of them is listed
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = {"soak": 900, "switch_cost": 900, "round_cost": 600}   # time limit of the leg's child process, seconds
COUNTERS = ("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt", "rounds")


def slab_bytes(site, t_max, k):
    """PolishWideLayout::slab_total of acn_qp_polwide.hpp, restated: bytes of one workgroup's slab"""
    N, Mg, nrow = int(site.N), int(site.Mg), int(site.M) + int(bool(site.has_peak))
    rows, sess = Mg * t_max, ((N * k + 7) // 8) * 8
    d = 8 * N * t_max + 2 * Mg * t_max + nrow * t_max + 5 * rows + t_max * (Mg * (Mg + 1) // 2) + Mg * N + sess * (sess + 1) // 2 + 12 * N
    d += (3 * rows + 1) // 2 + (2 * N * t_max + nrow * t_max + 4 * N + 7) // 8
    return 8 * ((d + 1) & ~1)


def soak_batch(n=None):
    """case 18 of tools/gpu_soak.py 512 8, built as that tool builds it (``n``: its first snapshots only)"""
    import numpy as np

    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites, tou_energy_cost, total_energy
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch
    from tests.test_gpu_parity import _random_sessions_general

    case, seed, T = 18, 8, 48
    rng = np.random.default_rng(5000 + case + 100 * seed)
    infra = sites.synth512()
    iface = Interface({"infrastructure_info": infra, "period": 5, "prices": rng.uniform(0.05, 0.4, size=256)})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 10.0 ** rng.uniform(-4, -2)),
           ObjectiveComponent(tou_energy_cost, float(rng.uniform(0, 5))), ObjectiveComponent(total_energy, float(rng.uniform(0, 2)))]
    snaps = [_random_sessions_general(infra, T, rng, False, min_rates=False, demand_scale=0.5 * 0.3) for _ in range(32)]
    return build_batch(snaps[:n], infra, iface, obj, "SOC", True, peak_limits=[None] * len(snaps[:n])), infra


def row_violation(infra, x):
    import numpy as np

    ph = np.deg2rad(infra.phases)
    cm = infra.constraint_matrix
    mag = np.hypot(np.einsum("mn,bnt->bmt", cm * np.cos(ph), x), np.einsum("mn,bnt->bmt", cm * np.sin(ph), x))
    return (mag - infra.constraint_limits[None, :, None]).max(axis=(1, 2))


def run_off_on(batch, options, launches, want_x=False):
    """lone device-resident launches, the two settings interleaved; per setting the launch times and the last launch's results"""
    import numpy as np
    import torch

    from adacharge_amd.backend import DeviceBatch, SiteHandle

    dev = torch.device("cuda", 0)
    handles = {"off": SiteHandle(batch.site, 0), "on": SiteHandle(batch.site, 0, polish_wide=True)}
    dbs = {k: DeviceBatch(batch, dev) for k in handles}
    stream = torch.cuda.current_stream().cuda_stream
    ms = {k: [] for k in handles}
    for k, h in handles.items():   # warm-up: code objects, workspaces, slabs
        h.solve_device(dbs[k], options, stream=stream)
        torch.cuda.synchronize()
        h.kernel_times()
    s0 = handles["on"].polish_stats()
    for _ in range(launches):
        for k, h in handles.items():
            h.solve_device(dbs[k], options, stream=stream)
            torch.cuda.synchronize()
            ms[k] += h.kernel_times()
    s1 = handles["on"].polish_stats()
    out, xs = {}, {}
    for k, h in handles.items():
        it, st = dbs[k].iters.cpu().numpy(), dbs[k].status.cpu().numpy()
        fam, pol = h.route(batch.Tm, batch.K, batch.B)
        t = sorted(ms[k])
        out[k] = {"family": fam, "polish": int(pol), "ms_median": round(float(np.median(t)), 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3),
                  "launches": len(t), "iters_mean": round(float(it.mean()), 1), "iters_max": int(it.max()),
                  "status": {str(int(v)): int(c) for v, c in zip(*np.unique(st, return_counts=True))}}
        xs[k] = (dbs[k].x.cpu().numpy(), st, it)
    rounds = s1["rounds"] - s0["rounds"]
    us = sum(s1["phase_us"]) - sum(s0["phase_us"])
    out["on"]["per_launch"] = {c: (s1[c] - s0[c]) / launches for c in COUNTERS}
    out["on"]["workgroup_us_per_round"] = round(us / rounds, 1) if rounds else None
    out["on"]["phase_us_share"] = [round((a - b) / max(1, us), 3) for a, b in zip(s1["phase_us"], s0["phase_us"])]
    out["on"]["slab_bytes_per_workgroup"] = slab_bytes(batch.site, batch.Tm, batch.K)
    out["shape"] = {"B": int(batch.B), "N": int(batch.N), "t_max": int(batch.Tm), "K": int(batch.K), "Mg": int(batch.site.Mg)}
    for h in handles.values():
        h.close()
    return (out, xs) if want_x else out


def leg_soak(launches):
    import numpy as np

    from adacharge_amd.backend import default_options

    batch, infra = soak_batch()
    out, xs = run_off_on(batch, default_options(max_iter=30000, polish_iters=800), 1, want_x=True)
    (x0, st0, it0), (x1, st1, it1) = xs["off"], xs["on"]
    open_ = [int(b) for b in np.flatnonzero(np.isin(st0, (2, 5)))]
    v0, v1 = row_violation(infra, x0), row_violation(infra, x1)
    out["listed"] = [{"problem": b, "status_off": int(st0[b]), "status_on": int(st1[b]), "iters_off": int(it0[b]), "iters_on": int(it1[b]),
                      "rounds": int(it1[b] - it0[b]), "row_violation_off_A": float(v0[b]), "row_violation_on_A": float(v1[b]),
                      "max_abs_dx_A": float(np.abs(x1[b] - x0[b]).max())} for b in open_]
    ok0, ok1 = np.isin(st0, (1, 5)), np.isin(st1, (1, 5))
    out["worst_row_violation_A"] = {"off": float(v0[ok0].max()) if ok0.any() else None, "on": float(v1[ok1].max()) if ok1.any() else None}
    rest = [b for b in range(batch.B) if b not in open_]
    out["others_bitwise_equal"] = bool(np.array_equal(x0[rest], x1[rest]) and np.array_equal(st0[rest], st1[rest]) and np.array_equal(it0[rest], it1[rest]))
    return out


def leg_switch_cost(launches):
    import numpy as np

    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import default_options
    from adacharge_amd.builder import ProblemBatch, build_batch, scenario_batch

    infra = sites.synth512()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
    rng = np.random.default_rng(5)
    snaps = [sites.random_sessions_general(infra, 48, rng, False, False, demand_scale=0.12) for _ in range(8)]
    base = build_batch(snaps, infra, iface, obj, "SOC", True)
    batch = ProblemBatch.concatenate([scenario_batch(base, rng.lognormal(0.0, 0.05, size=256), problem=p) for p in range(8)])
    out = run_off_on(batch, default_options(), launches)
    out["ms_median_on_minus_off"] = round(out["on"]["ms_median"] - out["off"]["ms_median"], 3)
    return out


def leg_round_cost(launches):
    from adacharge_amd.backend import default_options

    batch, _ = soak_batch(4)
    return run_off_on(batch, default_options(max_iter=800, eps_abs=1e-30, eps_rel=1e-30, retry_passes=0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polish_wide.json"))
    ap.add_argument("--leg", default=None, help="(a child process: run this leg and print its JSON)")
    ap.add_argument("legs", nargs="*")
    a = ap.parse_args()
    if a.leg:
        print("LEG_JSON " + json.dumps(globals()["leg_" + a.leg](a.launches)), flush=True)
        return 0
    import torch

    res = {"device": torch.cuda.get_device_name(0), "launches": a.launches, "legs": {}}
    for name in a.legs or list(LEGS):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--launches", str(a.launches)], cwd=ROOT,
                               stdout=subprocess.PIPE, text=True, timeout=LEGS[name])
        except subprocess.TimeoutExpired:
            print(f"leg {name}: no result within {LEGS[name]} s; stopping", flush=True)
            return 1
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LEG_JSON ")), None)
        if r.returncode != 0 or line is None:
            print(f"leg {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", flush=True)
            return 1
        res["legs"][name] = json.loads(line[len("LEG_JSON "):])
        print(json.dumps({name: res["legs"][name]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:   # (after every leg: a run that is cut short keeps what it has)
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
