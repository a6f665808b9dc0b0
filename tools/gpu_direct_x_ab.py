"""A/B of the direct path for x and the chunk plan without a small last chunk (acn_qp_pipeline.hpp, DESIGN.md section
3.7) against the parent commit's library, on one MI355X, by the protocol of tools/gpu_order_key_ab.py: fresh child
processes, one at a time, each under its own time limit, the two builds alternating (and alternating who goes first);
the script stops at the first child that faults, aborts or times out (any non-zero exit).

    python tools/gpu_direct_x_ab.py <parent library> [--record profiles/direct_x_ab.json] [--turns 5] [--phase plain|full|both] [--budget SECONDS]

`this` is the library of the tree (ACNQP_LIBRARY unset), `parent` the library given.  plain: `python bench.py` (the headline
step); turn 0 of either build also dumps its outputs (--dump-outputs), and the dumps are compared file by file.  full:
`python bench.py --full --no-cpu-baseline`.  Recorded: every run's ms_per_step, kernel_only.launch_ms,
strict_batch256.ms_per_call_median, host_inclusive.table.solve_table_ms and every other_configs leg's kernel_ms.
A figure is a GAIN only if this build's slowest run beats the parent's fastest, a LOSS if its fastest run is slower than
the parent's slowest.  A phase run on its own keeps the other phase's entries of an existing record, and the record is
rewritten after every turn.  --budget: no further turn starts once the phases' time so far plus 1.2 x the longest turn
would exceed it; the record then says how many turns were completed.  The exit status is 1 if a dump differs."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PLAIN_TIMEOUT, FULL_TIMEOUT = 120, 300   # seconds per child
SWITCHES = ("ACNQP_NO_DIRECT_X", "ACNQP_PLAN", "ACNQP_CHUNK", "ACNQP_NO_RAMP", "ACNQP_NO_STAGING", "ACNQP_NO_ORDER", "ACNQP_NO_QUEUE")


def run(lib, args, limit):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("ACNQP_LIBRARY",)}
    if lib:
        env["ACNQP_LIBRARY"] = lib
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       check=True, env=env, stdout=subprocess.PIPE, text=True)   # (the first non-zero exit ends the run)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def verdict(this, parent):
    return {"parent": {"runs": parent, "min": min(parent), "max": max(parent)}, "this": {"runs": this, "min": min(this), "max": max(this)},
            "gain": max(this) < min(parent), "loss": min(this) > max(parent)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_library")
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "direct_x_ab.json"))
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--phase", default="both", choices=["plain", "full", "both"])
    ap.add_argument("--budget", type=float, default=0.0, help="seconds this invocation may take (0: no limit)")
    args = ap.parse_args()
    from adacharge_amd.backend import library_path

    builds = [("parent", os.path.abspath(args.parent_library)), ("this", None)]
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
    out = json.load(open(args.record)) if os.path.exists(args.record) else {}
    out.update(turns_per_build=args.turns, rule="gain: this build's slowest run beats the parent's fastest; loss: the mirror image",
               library_sha256={"parent": sha(builds[0][1]), "this": sha(library_path())})
    same = {}
    t_start, longest = time.monotonic(), [0.0]

    def room(t_turn):
        """called after a turn that began at t_turn: whether another one fits the budget"""
        longest[0] = max(longest[0], time.monotonic() - t_turn)
        return args.budget <= 0 or time.monotonic() - t_start + 1.2 * longest[0] <= args.budget

    def save():
        with open(args.record, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if args.phase in ("plain", "both"):
        tmp = tempfile.mkdtemp(prefix="direct_x_ab_")
        ms = {"parent": [], "this": []}
        for turn in range(args.turns):
            t_turn = time.monotonic()
            for tag, lib in (builds if turn % 2 == 0 else builds[::-1]):
                j = run(lib, ["--dump-outputs", os.path.join(tmp, tag)] if turn == 0 else [], PLAIN_TIMEOUT)
                ms[tag].append(j["ms_per_step"])
                print(f"[ab] plain turn {turn} {tag}: {j['ms_per_step']:.3f} ms per step", flush=True)
            out["plain"] = {"command": "python bench.py", "turns_completed": turn + 1, "ms_per_step": verdict(ms["this"], ms["parent"])}
            save()
            if not room(t_turn):
                break
        names = sorted(set(os.listdir(os.path.join(tmp, "parent"))) | set(os.listdir(os.path.join(tmp, "this"))))
        for name in names:
            a, b = (os.path.join(tmp, t, name) for t in ("parent", "this"))
            same[name] = os.path.exists(a) and os.path.exists(b) and sha(a) == sha(b)
        shutil.rmtree(tmp)
        out["plain"]["dump_outputs_equal_to_parent"] = same
    if args.phase in ("full", "both"):
        recs = {"parent": [], "this": []}
        longest[0] = 0.0
        t_start = time.monotonic()
        for turn in range(args.turns):
            t_turn = time.monotonic()
            for tag, lib in (builds if turn % 2 == 0 else builds[::-1]):
                j = run(lib, ["--full", "--no-cpu-baseline"], FULL_TIMEOUT)
                rec = {"ms_per_step": j["ms_per_step"], "kernel_only.launch_ms": j["kernel_only"]["launch_ms"],
                       "strict_batch256.ms_per_call_median": j["strict_batch256"]["ms_per_call_median"],
                       "host_inclusive.table.solve_table_ms": j["host_inclusive"]["table"]["solve_table_ms"]}
                rec.update({"other_configs." + leg + ".kernel_ms": v["kernel_ms"] for leg, v in j["other_configs"].items()})
                recs[tag].append(rec)
                print(f"[ab] full turn {turn} {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in rec.items()), flush=True)
            out["full"] = {"command": "python bench.py --full --no-cpu-baseline", "turns_completed": turn + 1}
            for key in recs["this"][0]:
                out["full"][key] = verdict([r[key] for r in recs["this"]], [r[key] for r in recs["parent"]])
            save()
            if not room(t_turn):
                break
    save()
    print(json.dumps({ph: {k: ("gain" if v["gain"] else "loss" if v["loss"] else "neither", v["parent"]["min"], v["parent"]["max"], v["this"]["min"], v["this"]["max"])
                           for k, v in out.get(ph, {}).items() if isinstance(v, dict) and "gain" in v} for ph in ("plain", "full")}))
    raise SystemExit(0 if all(same.values()) else 1)
