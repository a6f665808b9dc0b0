"""Wall-clock A/B of the post-solve HOST entries between two builds of libacn_qp_hip.so: one ``h.duals(batch, res)`` at
16,384 x 54 x 12 and one ``h.pilots(plan, x)`` (REALLOCATE) at the shape of tools/gpu_pilots.py, the same solved batch
for both.  One child process per library and turn (ACNQP_LIBRARY selects the library, as in tools/gpu_ab_library.py), one
at a time, each under its own time limit, the two libraries alternating and each going first once: other, this, this,
other.  A child makes one warm-up call and five timed calls of each entry and prints their times and a sha256 of the
outputs.

    python tools/gpu_post_stage_ab.py child                           one library (ACNQP_LIBRARY): a JSON line
    python tools/gpu_post_stage_ab.py <other.so> [record.json]        both, alternating; the record (default
                                                                      profiles/post_stage_ab.json) holds every time, the
                                                                      median and the min-max spread of each build's ten
                                                                      calls, and whether the outputs agree bit for bit

Nothing is asserted about any time; the exit status is 1 if the outputs of the two builds differ."""
import hashlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, HORIZON, CALLS, TURNS = 16384, 12, 5, 2
CHILD_TIMEOUT = 240   # seconds per child


def child():
    import numpy as np
    from adacharge_amd import ObjectiveComponent, equal_share, postprocessing as pp, quick_charge, sites
    from adacharge_amd import session_table as st
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import plan_from_table

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    table = st.enforce_pilot_limit(sites.snapshot_table(infra, HORIZON, BATCH), infra)
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    batch = plan_from_table(table, infra, iface, obj, "SOC", False, None).expand()
    h = SiteHandle(batch.site, 0)
    res = h.solve(batch, default_options(), want_y=True)
    plan = pp.pilot_plan_arrays(table, infra, iface, "reallocate", batch=batch.B, t_max=batch.Tm)

    def timed(call):
        out = call()   # warm-up: the staging buffer grows here
        times = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            out = call()
            times.append((time.perf_counter() - t0) * 1e3)
        return times, out

    d_ms, d = timed(lambda: h.duals(batch, res))
    p_ms, p = timed(lambda: h.pilots(plan, res.x))
    h.close()
    sha = hashlib.sha256()
    for a in (d.mu, d.z, d.stat, d.energy, d.site, d.comp, *p):
        sha.update(np.ascontiguousarray(a).tobytes())
    print(json.dumps({"shape": [int(batch.B), int(batch.N), int(batch.Tm)], "duals_ms": d_ms, "pilots_ms": p_ms, "sha256": sha.hexdigest(),
                      "solved": int(np.isin(res.status, (1, 5)).sum())}))


def summary(runs):
    flat = [t for r in runs for t in r]
    return {"median": statistics.median(flat), "min": min(flat), "max": max(flat), "runs": runs}


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child()
        raise SystemExit(0)
    from adacharge_amd.build import LIB

    other = os.path.abspath(sys.argv[1])
    record = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "post_stage_ab.json")
    got = {"other": [], "this": []}
    order = []
    for turn in range(TURNS):
        for tag, lib in (("other", other), ("this", LIB))[::1 if turn % 2 == 0 else -1]:
            order.append(tag)
            env = dict(os.environ)
            env["ACNQP_LIBRARY"] = lib
            env.pop("ACNQP_POST_CHUNK", None)
            r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "child"],
                               check=True, env=env, stdout=subprocess.PIPE, text=True)   # (the first non-zero exit ends the run)
            got[tag].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"[ab] turn {turn} {tag}: duals {statistics.median(got[tag][-1]['duals_ms']):.1f} ms, pilots {statistics.median(got[tag][-1]['pilots_ms']):.1f} ms", flush=True)
    shas = {c["sha256"] for v in got.values() for c in v}
    out = {"shape": got["this"][0]["shape"], "calls_per_child": CALLS, "order": order, "same_bits": len(shas) == 1}
    for tag, path in (("other", other), ("this", LIB)):
        out[tag] = {"library": os.path.basename(path) if tag == "other" else os.path.relpath(path, ROOT),
                    "sha256": hashlib.sha256(open(path, "rb").read()).hexdigest(),
                    "duals_host_ms": summary([c["duals_ms"] for c in got[tag]]), "pilots_host_ms": summary([c["pilots_ms"] for c in got[tag]])}
    for key in ("duals_host_ms", "pilots_host_ms"):
        out[key.replace("_ms", "_this_median_within_other_spread")] = out["other"][key]["min"] <= out["this"][key]["median"] <= out["other"][key]["max"]
    with open(record, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in ("other", "this")}))
    raise SystemExit(0 if out["same_bits"] else 1)
