"""A/B of this build against the parent commit's for the polish launch alongside the solver (DESIGN.md sections 2.3 and
3.7), by the protocol of tools/gpu_wave_trim_ab.py: one child process per build and turn (ACNQP_LIBRARY selects the
library), one at a time, each under its own time limit, the builds alternating who goes first.

    python tools/gpu_polish_alongside_ab.py <parent build's libacn_qp_hip.so> [record.json] [turns] [plain|full|both]

(`plain` / `full`: one of the two commands only, merged into an existing record of the same two libraries.)

Five turns each of `python bench.py` (turn 0 of either build also dumps its outputs, compared file by file) and of
`python bench.py --full --no-cpu-baseline`.  Recorded per run: ms_per_step of both commands, kernel_only.launch_ms, the
other_configs legs and strict_batch256.ms_per_call_median.  `gain`: this build's SLOWEST run beats the parent's FASTEST;
`loss`: the parent's slowest beats this build's fastest.  The exit status is 1 if a dump differs."""
import hashlib, json, os, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adacharge_amd.build import LIB  # noqa: E402

LEGS = {"cfg2_jpl52": "cfg2_jpl52_T24_b4096", "cfg2_caltech54": "cfg2_caltech54_T24_b4096", "cfg3_site3": "cfg3_site3_T12_b1024", "cfg3_site0": "cfg3_site0_T12_b1024"}
PLAIN_TIMEOUT, FULL_TIMEOUT = 120, 240   # seconds per child
SWITCHES = ("ACNQP_NO_POLISH_ALONGSIDE", "ACNQP_POLISH_ALONGSIDE_SPINS", "ACNQP_POLISH_ALONGSIDE_GRID")


def run(lib, args, limit):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ACNQP_LIBRARY=lib)
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       check=True, env=env, stdout=subprocess.PIPE, text=True)   # (the first non-zero exit ends the run)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def verdict(vals, parent_vals):
    return {"runs": vals, "min": min(vals), "max": max(vals), "gain": max(vals) < min(parent_vals), "loss": max(parent_vals) < min(vals)}


if __name__ == "__main__":
    parent_lib = os.path.abspath(sys.argv[1])
    record = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "polish_alongside_ab.json")
    turns = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    phase = sys.argv[4] if len(sys.argv) > 4 else "both"
    builds = [("parent", parent_lib), ("this", LIB)]
    out = {"turns_per_build": turns, "rule": "gain: this build's slowest run beats the parent's fastest; loss: the parent's slowest beats this build's fastest",
           "builds": {tag: {"library_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest()} for tag, lib in builds}}
    if phase != "both" and os.path.exists(record):
        with open(record) as f:
            old = json.load(f)
        if old.get("builds") == out["builds"] and old.get("turns_per_build") == turns:
            out = old
    tmp = tempfile.mkdtemp(prefix="polish_alongside_ab_")
    plain = {tag: [] for tag, _ in builds}
    full = {tag: [] for tag, _ in builds}
    for turn in range(turns if phase in ("plain", "both") else 0):
        k = turn % 2
        for tag, lib in builds[k:] + builds[:k]:
            j = run(lib, ["--dump-outputs", os.path.join(tmp, tag)] if turn == 0 else [], PLAIN_TIMEOUT)
            plain[tag].append(j["ms_per_step"])
            print(f"[ab] plain turn {turn} {tag}: {j['ms_per_step']:.3f} ms per step", flush=True)
    for turn in range(turns if phase in ("full", "both") else 0):
        k = turn % 2
        for tag, lib in builds[k:] + builds[:k]:
            j = run(lib, ["--full", "--no-cpu-baseline"], FULL_TIMEOUT)
            rec = {"ms_per_step": j["ms_per_step"], "kernel_only.launch_ms": j["kernel_only"]["launch_ms"],
                   "strict_batch256.ms_per_call_median": j["strict_batch256"]["ms_per_call_median"]}
            rec.update({short: j["other_configs"][leg]["kernel_ms"] for short, leg in LEGS.items()})
            full[tag].append(rec)
            print(f"[ab] full turn {turn} {tag}: " + ", ".join(f"{k_} {v:.3f}" for k_, v in rec.items()), flush=True)
    def strip(block):
        for v in block.values():
            if isinstance(v, dict):
                v["parent"].pop("gain"), v["parent"].pop("loss")

    if plain["parent"]:
        same = {}
        for name in sorted(os.listdir(os.path.join(tmp, "parent"))):
            a, b = (hashlib.sha256(open(os.path.join(tmp, t, name), "rb").read()).hexdigest() for t in ("parent", "this"))
            same[name] = a == b
        out["dump_outputs_equal_to_parent"] = same
        out["plain"] = {"command": "python bench.py", "ms_per_step": {tag: verdict(plain[tag], plain["parent"]) for tag, _ in builds}}
        strip(out["plain"])
    shutil.rmtree(tmp)
    if full["parent"]:
        out["full"] = {"command": "python bench.py --full --no-cpu-baseline"}
        for key in full["parent"][0]:
            pv = [r[key] for r in full["parent"]]
            out["full"][key] = {tag: verdict([r[key] for r in full[tag]], pv) for tag, _ in builds}
        strip(out["full"])
    with open(record, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    same = out.get("dump_outputs_equal_to_parent", {})
    print(json.dumps({"dumps_equal": bool(same) and all(same.values()),
                      "figures": {k: {t: (v[t].get("gain"), v[t].get("loss"), v[t]["min"], v[t]["max"]) for t in v}
                                  for blk in ("plain", "full") for k, v in out.get(blk, {}).items() if isinstance(v, dict)}}))
    raise SystemExit(0 if (not plain["parent"]) or (same and all(same.values())) else 1)
