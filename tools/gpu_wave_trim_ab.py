"""A/B of several builds of the library against the parent's -- how the wave kernel's EVSE extent (shipped) and an Anderson
ring write by scalar dispatch (measured slower, not shipped) were told apart -- by the
protocol of tools/gpu_wave_rank_ab.py: one child process per build and turn (ACNQP_LIBRARY selects the library), one at a
time, each under its own time limit, the builds rotating who goes first.

    python tools/gpu_wave_trim_ab.py plain <record.json> <turns> tag=lib[,KEY=VALUE...] ...
    python tools/gpu_wave_trim_ab.py full  <record.json> <turns> tag=lib[,KEY=VALUE...] ...

The first build listed is the parent.  KEY=VALUE pairs go into that build's environment (ACNQP_WAVE_FULL_EVSE=1: a build
without its EVSE extent).  `plain`: `python bench.py` (the headline step); turn 0 of every build also dumps its
outputs (--dump-outputs), and every dump is compared with the parent's file by file.  `full`: `python bench.py --full
--no-cpu-baseline` (the lone launch and the other_configs legs).  `gain` is true for a figure only if that build's
SLOWEST run beats the parent's FASTEST.  The exit status is 1 if a dump differs."""
import hashlib, json, os, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGS = ("cfg3_site3_T12_b1024", "cfg3_site0_T12_b1024", "cfg2_caltech54_T24_b4096", "cfg2_jpl52_T24_b4096")
PLAIN_TIMEOUT, FULL_TIMEOUT = 120, 240   # seconds per child


def run(lib, extra_env, args, limit):
    env = {k: v for k, v in os.environ.items() if k not in ("ACNQP_WAVE_FULL_RANK", "ACNQP_WAVE_FULL_EVSE", "ACNQP_NO_WAVE", "ACNQP_NO_WAVE2")}
    env.update(extra_env, ACNQP_LIBRARY=lib)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       check=True, env=env, stdout=subprocess.PIPE, text=True)   # (the first non-zero exit ends the run)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def spread(vals, parent_vals):
    return {"runs": vals, "min": min(vals), "max": max(vals), "gain": max(vals) < min(parent_vals)}


if __name__ == "__main__":
    phase, record, turns = sys.argv[1], sys.argv[2], int(sys.argv[3])
    builds = []
    for spec in sys.argv[4:]:
        tag, rest = spec.split("=", 1)
        lib, *pairs = rest.split(",")
        builds.append((tag, os.path.abspath(lib), dict(p.split("=", 1) for p in pairs)))
    parent = builds[0][0]
    out = {"turns_per_build": turns, "rule": "gain: the build's slowest run beats the parent's fastest",
           "builds": {tag: {"library_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest(), "environment": env} for tag, lib, env in builds}}
    same = {}
    if phase == "plain":
        out["command"] = "python bench.py"
        tmp = tempfile.mkdtemp(prefix="wave_trim_ab_")
        ms = {tag: [] for tag, _, _ in builds}
        for turn in range(turns):
            k = turn % len(builds)
            for tag, lib, env in builds[k:] + builds[:k]:
                extra = ["--dump-outputs", os.path.join(tmp, tag)] if turn == 0 else []
                j = run(lib, env, extra, PLAIN_TIMEOUT)
                ms[tag].append(j["ms_per_step"])
                print(f"[ab] plain turn {turn} {tag}: {j['ms_per_step']:.3f} ms per step", flush=True)
        for tag, _, _ in builds[1:]:
            same[tag] = {}
            for name in sorted(os.listdir(os.path.join(tmp, parent))):
                a, b = (hashlib.sha256(open(os.path.join(tmp, t, name), "rb").read()).hexdigest() for t in (parent, tag))
                same[tag][name] = a == b
        shutil.rmtree(tmp)
        out["dump_outputs_equal_to_parent"] = same
        out["plain_ms_per_step"] = {tag: spread(ms[tag], ms[parent]) for tag, _, _ in builds}
        out["plain_ms_per_step"][parent].pop("gain")
    else:
        out["command"] = "python bench.py --full --no-cpu-baseline"
        full = {tag: [] for tag, _, _ in builds}
        for turn in range(turns):
            k = turn % len(builds)
            for tag, lib, env in builds[k:] + builds[:k]:
                j = run(lib, env, ["--full", "--no-cpu-baseline"], FULL_TIMEOUT)
                rec = {"ms_per_step": j["ms_per_step"], "launch_ms": j["kernel_only"]["launch_ms"]}
                rec.update({leg: j["other_configs"][leg]["kernel_ms"] for leg in LEGS})
                full[tag].append(rec)
                print(f"[ab] full turn {turn} {tag}: " + ", ".join(f"{k_} {v:.3f}" for k_, v in rec.items()), flush=True)
        for key in ("ms_per_step", "launch_ms") + LEGS:
            pv = [r[key] for r in full[parent]]
            out["full_" + key] = {tag: spread([r[key] for r in full[tag]], pv) for tag, _, _ in builds}
            out["full_" + key][parent].pop("gain")
    with open(record, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {t: (v[t].get("gain"), v[t]["min"], v[t]["max"]) for t in v} for k, v in out.items() if k.startswith(("plain_", "full_"))}))
    raise SystemExit(0 if all(all(d.values()) for d in same.values()) else 1)
