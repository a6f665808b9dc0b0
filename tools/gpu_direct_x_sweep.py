"""Sweep of chunk plans for the headline step with the direct path for x, on one MI355X: every
candidate is an explicit ACNQP_PLAN, measured by fresh child processes of `python bench.py`, one at a time, each under its
own time limit; the rounds go through all candidates in turn, so that drift hits them alike.  The script stops at the
first child that faults, aborts or times out (any non-zero exit).

    python tools/gpu_direct_x_sweep.py [--record profiles/direct_x_plan_sweep.json] [--runs 3] [--budget SECONDS] [name=plan ...]

A candidate `name=a,b,c` sets ACNQP_PLAN=a,b,c (the rest of the call goes into a last chunk); `name=` leaves the planner's
default; a name that ends in `!copy` also sets ACNQP_NO_DIRECT_X=1 (the copy path, in the same binary).  Default
candidates: the plans of the issue for 16,384 problems (c = 8,192).  --budget: no further round starts once the time so far
plus 1.2 x the longest round would exceed it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 120   # seconds per child
DEFAULT = ("default=", "c/4,c/4,c/2,c=2048,2048,4096", "3c/16,5c/16,c/2,c=1536,2560,4096", "c/4,c/2,c/2,3c/4=2048,4096,4096",
           "c/4,c/2,c,c/4=2048,4096,8192", "c/4,c/2,c,c/4!copy=2048,4096,8192")


def run(name, plan):
    env = {k: v for k, v in os.environ.items() if k not in ("ACNQP_PLAN", "ACNQP_NO_DIRECT_X", "ACNQP_CHUNK", "ACNQP_LIBRARY")}
    if plan:
        env["ACNQP_PLAN"] = plan
    if name.endswith("!copy"):
        env["ACNQP_NO_DIRECT_X"] = "1"
    r = subprocess.run(["timeout", "-k", "10", str(TIMEOUT), sys.executable, os.path.join(ROOT, "bench.py")],
                       check=True, env=env, stdout=subprocess.PIPE, text=True)
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["ms_per_step"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("candidates", nargs="*", default=list(DEFAULT))
    ap.add_argument("--record", default=os.path.join(ROOT, "profiles", "direct_x_plan_sweep.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--budget", type=float, default=0.0)
    args = ap.parse_args()
    cands = [c.split("=", 1) for c in args.candidates]
    out = {"command": "python bench.py", "problems_per_call": 16384, "runs_per_candidate": 0,
           "candidates": {n: {"ACNQP_PLAN": p or None, "ACNQP_NO_DIRECT_X": n.endswith("!copy"), "ms_per_step": []} for n, p in cands}}
    t_start, longest = time.monotonic(), 0.0
    for k in range(args.runs):
        t0 = time.monotonic()
        for n, p in (cands if k % 2 == 0 else cands[::-1]):
            out["candidates"][n]["ms_per_step"].append(run(n, p))
            print(f"[sweep] round {k} {n}: {out['candidates'][n]['ms_per_step'][-1]:.3f} ms per step", flush=True)
        out["runs_per_candidate"] = k + 1
        with open(args.record, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        longest = max(longest, time.monotonic() - t0)
        if args.budget > 0 and time.monotonic() - t_start + 1.2 * longest > args.budget:
            break
    print(json.dumps({n: [min(v["ms_per_step"]), max(v["ms_per_step"])] for n, v in out["candidates"].items()}))
