"""A/B of the wave kernel's eigen extent between two builds of libacn_qp_hip.so: the parent's (given) and this tree's.

    python tools/gpu_wave_rank_ab.py <parent.so> [record.json] [turns]

One child process per library and turn (ACNQP_LIBRARY selects the library, as in tools/gpu_ab_library.py), one at a time,
each under its own time limit, the two libraries alternating and taking turns at going first:
  * `python bench.py` (the headline step); turn 0 of each library also dumps its outputs (--dump-outputs), and the two
    dumps are compared file by file -- the inputs depend on the arguments only, so equal files mean equal bits;
  * `python bench.py --full --no-cpu-baseline` (the lone launch `kernel_only.launch_ms` and the other_configs legs).
The record (default profiles/wave_rank_ab.json) holds every run.  `gain` is true for a figure only if this build's SLOWEST
run beats the parent's FASTEST.  The exit status is 1 if the dumps differ."""
import hashlib, json, os, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("cfg3_site3_T12_b1024", "cfg3_site0_T12_b1024", "cfg2_caltech54_T24_b4096", "cfg2_jpl52_T24_b4096")
PLAIN_TIMEOUT, FULL_TIMEOUT = 120, 240   # seconds per child


def run(lib, args, limit):
    env = dict(os.environ, ACNQP_LIBRARY=lib)
    for k in ("ACNQP_WAVE_FULL_RANK", "ACNQP_NO_WAVE", "ACNQP_NO_WAVE2"):
        env.pop(k, None)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       check=True, env=env, stdout=subprocess.PIPE, text=True)   # (the first non-zero exit ends the run)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def spread(vals, parent_vals):
    return {"runs": vals, "min": min(vals), "max": max(vals), "gain": max(vals) < min(parent_vals)}


if __name__ == "__main__":
    from adacharge_amd.build import LIB

    parent = os.path.abspath(sys.argv[1])
    record = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "wave_rank_ab.json")
    turns = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    libs = (("parent", parent), ("this", LIB))
    tmp = tempfile.mkdtemp(prefix="wave_rank_ab_")
    plain = {"parent": [], "this": []}
    full = {"parent": [], "this": []}
    for turn in range(turns):
        for tag, lib in libs[::1 if turn % 2 == 0 else -1]:
            extra = ["--dump-outputs", os.path.join(tmp, tag)] if turn == 0 else []
            j = run(lib, extra, PLAIN_TIMEOUT)
            plain[tag].append(j["ms_per_step"])
            print(f"[ab] plain turn {turn} {tag}: {j['ms_per_step']:.3f} ms per step", flush=True)
    same = {}
    for name in sorted(os.listdir(os.path.join(tmp, "parent"))):
        a, b = (hashlib.sha256(open(os.path.join(tmp, tag, name), "rb").read()).hexdigest() for tag in ("parent", "this"))
        same[name] = a == b
    shutil.rmtree(tmp)
    print(f"[ab] dumps equal: {same}", flush=True)
    for turn in range(turns):
        for tag, lib in libs[::-1 if turn % 2 == 0 else 1]:
            j = run(lib, ["--full", "--no-cpu-baseline"], FULL_TIMEOUT)
            rec = {"ms_per_step": j["ms_per_step"], "launch_ms": j["kernel_only"]["launch_ms"]}
            rec.update({leg: j["other_configs"][leg]["kernel_ms"] for leg in LEGS})
            full[tag].append(rec)
            print(f"[ab] full turn {turn} {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in rec.items()), flush=True)
    out = {"commands": ["python bench.py", "python bench.py --full --no-cpu-baseline"], "turns_per_build": turns,
           "rule": "gain: this build's slowest run beats the parent's fastest", "dump_outputs_equal": same,
           "libraries": {tag: hashlib.sha256(open(lib, "rb").read()).hexdigest() for tag, lib in libs}}
    out["plain_ms_per_step"] = {"parent": spread(plain["parent"], plain["parent"]), "this": spread(plain["this"], plain["parent"])}
    out["plain_ms_per_step"]["parent"].pop("gain")
    for key in ("ms_per_step", "launch_ms") + LEGS:
        pv, tv = [r[key] for r in full["parent"]], [r[key] for r in full["this"]]
        out["full_" + key] = {"parent": {"runs": pv, "min": min(pv), "max": max(pv)}, "this": spread(tv, pv)}
    with open(record, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["this"]["gain"], v["parent"]["min"], v["this"]["max"]) for k, v in out.items() if isinstance(v, dict) and isinstance(v.get("this"), dict)}))
    raise SystemExit(0 if all(same.values()) else 1)
