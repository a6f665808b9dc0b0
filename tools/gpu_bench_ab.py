"""A/B of builds of the library on bench.py, on one MI355X: the one protocol by which a performance change is accepted or
rejected.  Fresh child processes, one at a time, each `timeout -k 10 <limit> python bench.py ...`; in turn k the builds
run rotated by k mod n (two builds alternate who goes first); the first child that exits non-zero (a time limit, an
abort, a fault) ends the whole run: no further child starts, the record as last written stays, the exit status is 2.

    python tools/gpu_bench_ab.py [--record FILE] [--turns 5] [--phase plain|full|both] [--budget SECONDS] tag=[lib][,KEY=VALUE...] ...

Builds.  The first build listed is the parent.  An empty `lib` is the tree's own library (ACNQP_LIBRARY unset for that
child).  A build's text after `tag=` is split at every comma that is followed by NAME= with NAME an upper-case identifier
([A-Z_][A-Z0-9_]*); the first piece is the library, the others are KEY=VALUE pairs of that build's children only, so commas
inside a value survive: `copy=,ACNQP_PLAN=2048,4096,8192,ACNQP_NO_DIRECT_X=1`.  A child's environment is the caller's
without EVERY variable that begins ACNQP_, plus the build's pairs, plus ACNQP_LIBRARY where the build names a library.
--record defaults to profiles/bench_ab.json for the parent and one build and is required for more.

Phases.  plain: `python bench.py`, the figure ms_per_step; in turn 0 every build also gets --dump-outputs <tmp>/<tag>, and
for every other build each file name on either side is true only if both files exist with equal sha256 (exit status 1 if
one is false).  full: `python bench.py --full --no-cpu-baseline`, the figures of FULL_FIGURES and other_configs.<leg>.kernel_ms
of every leg the JSON holds.  Per figure and build but the parent -- gain: the build's max is below the parent's min;
loss: its min is above the parent's max (equality is neither).

--budget: one clock for the invocation; no further turn starts once the time so far plus 1.2 x the longest turn of the
current phase would exceed it, no turn is left half done, and the record holds turns_completed per phase.  The record
(one layout: `builds`, `plain`, `full`) is rewritten after every completed turn; a phase run on its own keeps the other
phase's block of an existing record only if that record's `builds` block (tags, sha256, environments) equals this one's."""
import argparse
import collections
import functools
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
PHASES = {"plain": ([], 120), "full": (["--full", "--no-cpu-baseline"], 300)}   # bench.py's arguments, seconds per child
FULL_FIGURES = ("ms_per_step", "kernel_only.launch_ms", "strict_batch256.ms_per_call_median", "host_inclusive.table.solve_table_ms")
RULE = "gain: the build's slowest run beats the parent's fastest; loss: its fastest run is slower than the parent's slowest"
Build = collections.namedtuple("Build", "tag lib env")


def parse_builds(specs):
    builds = []
    for spec in specs:
        tag, eq, rest = spec.partition("=")
        if not (tag and eq) or tag in [b.tag for b in builds]:
            raise ValueError(f"build {spec!r}: expected tag=[lib][,KEY=VALUE...] with a tag of its own")
        lib, *pairs = re.split(r",(?=[A-Z_][A-Z0-9_]*=)", rest)
        builds.append(Build(tag, os.path.abspath(lib) if lib else None, dict(p.split("=", 1) for p in pairs)))
    return builds


def child_env(build, environ):
    env = {k: v for k, v in environ.items() if not k.startswith("ACNQP_")}
    env.update(build.env)
    if build.lib:
        env["ACNQP_LIBRARY"] = build.lib
    return env


def run_child(build, args, limit, program=BENCH):
    """one child: its JSON line, the last stdout line that begins with `{`; subprocess.CalledProcessError on a non-zero exit"""
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, program, *args],
                       check=True, env=child_env(build, os.environ), stdout=subprocess.PIPE, text=True)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def rotation(builds, turn):
    k = turn % len(builds)
    return builds[k:] + builds[:k]


def figures(phase, j):
    if phase == "plain":
        return {"ms_per_step": j["ms_per_step"]}
    out = {path: functools.reduce(lambda d, k: d[k], path.split("."), j) for path in FULL_FIGURES}
    out.update({f"other_configs.{leg}.kernel_ms": v["kernel_ms"] for leg, v in j["other_configs"].items()})
    return out


def verdicts(runs, parent):
    """runs: {tag: [values]} of one figure -> {tag: runs, min, max and, but for the parent, gain and loss}"""
    out = {tag: {"runs": v, "min": min(v), "max": max(v)} for tag, v in runs.items()}
    for tag, v in out.items():
        if tag != parent:
            v.update(gain=v["max"] < out[parent]["min"], loss=v["min"] > out[parent]["max"])
    return out


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def compare_dumps(tmp, parent, tags):
    ls = lambda tag: set(os.listdir(os.path.join(tmp, tag))) if os.path.isdir(os.path.join(tmp, tag)) else set()
    same = {}
    for tag in tags:
        files = {name: [os.path.join(tmp, t, name) for t in (parent, tag)] for name in sorted(ls(parent) | ls(tag))}
        same[tag] = {name: all(map(os.path.exists, ab)) and sha256(ab[0]) == sha256(ab[1]) for name, ab in files.items()}
    return same


def drive(builds, record, turns=5, phase="both", budget=0.0, run=run_child, clock=time.monotonic, tree_library=None):
    """the whole protocol; run(build, bench.py's arguments, time limit) -> bench.py's JSON.  Returns the exit status."""
    if tree_library is None and not all(b.lib for b in builds):
        sys.path.insert(0, ROOT)
        from adacharge_amd.build import LIB as tree_library
    parent, tags = builds[0].tag, [b.tag for b in builds]
    out = {"rule": RULE, "builds": {b.tag: {"library_sha256": sha256(b.lib or tree_library), "environment": b.env} for b in builds}}
    if phase != "both" and os.path.exists(record):
        with open(record) as f:
            old = json.load(f)
        if old.get("builds") == out["builds"]:
            out = old

    def save():
        with open(record, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    t_start, tmp = clock(), tempfile.mkdtemp(prefix="bench_ab_")
    try:
        for ph in ("plain", "full") if phase == "both" else (phase,):
            args, limit = PHASES[ph]
            block = out[ph] = {"command": " ".join(["python bench.py", *args]), "turns_requested": turns, "turns_completed": 0, "figures": {}}
            runs, longest = {}, 0.0
            for turn in range(turns):
                t_turn = clock()
                if budget > 0 and t_turn - t_start + 1.2 * longest > budget:
                    break
                for b in rotation(builds, turn):
                    dump = ["--dump-outputs", os.path.join(tmp, b.tag)] if ph == "plain" and turn == 0 else []
                    got = figures(ph, run(b, args + dump, limit))
                    for key, v in got.items():
                        runs.setdefault(key, {t: [] for t in tags})[b.tag].append(v)
                    print(f"[ab] {ph} turn {turn} {b.tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in got.items()), flush=True)
                longest = max(longest, clock() - t_turn)
                block.update(turns_completed=turn + 1, figures={key: verdicts(r, parent) for key, r in runs.items()})
                if ph == "plain" and turn == 0:
                    block["dump_outputs_equal_to_parent"] = compare_dumps(tmp, parent, tags[1:])
                save()
            save()   # (a phase the budget left no turn for says so)
    except subprocess.CalledProcessError as e:
        print(f"[ab] a child exited with status {e.returncode}: no further child is started", flush=True)
        return 2
    finally:
        shutil.rmtree(tmp)
    print(json.dumps({ph: {key: {t: ("gain" if v.get("gain") else "loss" if v.get("loss") else "neither" if "gain" in v else "parent", v["min"], v["max"]) for t, v in fig.items()}
                           for key, fig in out[ph]["figures"].items()} for ph in ("plain", "full") if ph in out}))
    same = out.get("plain", {}).get("dump_outputs_equal_to_parent", {}) if phase != "full" else {}
    return 0 if all(all(d.values()) for d in same.values()) else 1


def main(argv=None, **how):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("builds", nargs="+", metavar="tag=[lib][,KEY=VALUE...]", help="the first one is the parent")
    ap.add_argument("--record", help="default profiles/bench_ab.json; required for more than the parent and one build")
    ap.add_argument("--turns", type=int, default=5)
    ap.add_argument("--phase", default="both", choices=["plain", "full", "both"])
    ap.add_argument("--budget", type=float, default=0.0, help="seconds this invocation may take (0: no limit)")
    args = ap.parse_args(argv)
    try:
        builds = parse_builds(args.builds)
    except ValueError as e:
        ap.error(str(e))
    if len(builds) < 2 or (len(builds) > 2 and not args.record):
        ap.error("give the parent and at least one build, and --record for more than one build")
    return drive(builds, args.record or os.path.join(ROOT, "profiles", "bench_ab.json"), args.turns, args.phase, args.budget, **how)


if __name__ == "__main__":
    raise SystemExit(main())
