"""The headline step's timeline from one rocprofv3 trace per build (no GPU needed to read them):

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python bench.py        (once per build)
    python tools/direct_x_timeline.py name=DIR [name=DIR ...] [--steps 32] [--record profiles/direct_x_timeline.json]

A step is a run of device activity (kernels and copies) without an idle gap of 100 us that holds at least four solver
launches -- wave-kernel launches with the step's largest grid; the resume launches behind the polish are smaller --; the
last `--steps` of them are the timed ones.  Per build, medians over those steps, in ms:
  first_input_copy_to_first_solver_start   start of the step's first host-to-device copy -> start of its first solver kernel
  last_solver_end_to_last_activity         end of the last solver kernel to end -> end of the step's last kernel or copy
  last_solver_launch_start                 start of the step's last solver launch, from the step's first activity
  step_activity                            first to last activity
  d2h_copies, d2h_copy_ms                  device-to-host copies per step and the sum of their durations
  h2d_copies, h2d_copy_ms                  host-to-device copies per step and the sum of their durations (the trace has no
                                           size column: the copies' time at the link's rate is what tells their bytes)
  last_input_copy_end                      end of the step's last host-to-device copy, from the step's first activity
  d2h_bytes                                the trace has no size column: 5,184 + 32 bytes per problem where x is copied
                                           back (more than 8 device-to-host copies in a step), 32 where only the small
                                           result arrays are"""
import argparse
import csv
import glob
import json
import os
import statistics

GAP_NS = 100_000
PROBLEMS, X_BYTES, SMALL_BYTES = 16384, 54 * 12 * 8, 32


def events(d):
    ev = []
    for path in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "K", r["Kernel_Name"], int(r["Grid_Size_X"])))
    for path in glob.glob(os.path.join(d, "**", "*_memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "C", r["Direction"], 0))
    return sorted(ev)


def steps_of(ev):
    out, cur, end = [], [], 0
    for e in ev:
        if cur and e[0] - end > GAP_NS:
            out.append(cur)
            cur = []
        end = e[1] if not cur else max(end, e[1])
        cur.append(e)
    out.append(cur)
    return out


def solver_launches(step):
    waves = [e for e in step if e[2] == "K" and "admm_wave_kernel" in e[3]]
    big = max((e[4] for e in waves), default=0)
    return [e for e in waves if e[4] == big]


def describe(d, n_steps):
    steps = [s for s in steps_of(events(d)) if len(solver_launches(s)) >= 4][-n_steps:]
    rows = {k: [] for k in ("first_input_copy_to_first_solver_start", "last_solver_end_to_last_activity", "last_solver_launch_start",
                            "step_activity", "d2h_copies", "d2h_copy_ms", "h2d_copies", "h2d_copy_ms", "last_input_copy_end")}
    for s in steps:
        t0, t1 = s[0][0], max(e[1] for e in s)
        sol = solver_launches(s)
        h2d = [e for e in s if e[2] == "C" and e[3].endswith("HOST_TO_DEVICE")]
        d2h = [e for e in s if e[2] == "C" and e[3].endswith("DEVICE_TO_HOST")]
        rows["first_input_copy_to_first_solver_start"].append((min(e[0] for e in sol) - min(e[0] for e in h2d)) / 1e6)
        rows["last_solver_end_to_last_activity"].append((t1 - max(e[1] for e in sol)) / 1e6)
        rows["last_solver_launch_start"].append((max(e[0] for e in sol) - t0) / 1e6)
        rows["step_activity"].append((t1 - t0) / 1e6)
        rows["d2h_copies"].append(len(d2h))
        rows["d2h_copy_ms"].append(sum(e[1] - e[0] for e in d2h) / 1e6)
        rows["h2d_copies"].append(len(h2d))
        rows["h2d_copy_ms"].append(sum(e[1] - e[0] for e in h2d) / 1e6)
        rows["last_input_copy_end"].append((max(e[1] for e in h2d) - t0) / 1e6)
    out = {k: round(statistics.median(v), 3) for k, v in rows.items()}
    out["steps"] = len(steps)
    out["solver_launches_per_step"] = statistics.median(len(solver_launches(s)) for s in steps)
    out["d2h_bytes"] = PROBLEMS * (SMALL_BYTES + (X_BYTES if out["d2h_copies"] > 8 else 0))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("traces", nargs="+", help="name=directory of one rocprofv3 run")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--record", default=None)
    args = ap.parse_args()
    out = {"command": "rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -- python bench.py (one run per build; the profiler "
                      "lengthens the step: compare the builds with each other, and take the step's length from profiles/direct_x_ab.json)",
           "medians_over_steps": args.steps, "builds": {}}
    for t in args.traces:
        name, d = t.split("=", 1)
        out["builds"][name] = describe(d, args.steps)
    text = json.dumps(out, indent=1)
    print(text)
    if args.record:
        with open(args.record, "w") as f:
            f.write(text + "\n")
