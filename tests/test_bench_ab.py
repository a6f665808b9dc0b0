"""The rules of tools/gpu_bench_ab.py, the one A/B driver for benchmark comparisons of library builds, held on the CPU:
a fake runner returns canned bench.py-shaped dictionaries (and writes dump files), a fake clock tells the time; only the
environment tests start a process, a stub program written to tmp_path."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gpu_bench_ab", os.path.join(ROOT, "tools", "gpu_bench_ab.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

LEGS = ("cfg3_site3_T12_b1024", "cfg2_jpl52_T24_b4096")
FULL_NAMES = {"ms_per_step", "kernel_only.launch_ms", "strict_batch256.ms_per_call_median", "host_inclusive.table.solve_table_ms"}


def bench_json(ms, full, legs=LEGS):
    j = {"metric": "ms_per_step", "ms_per_step": ms, "solved": 16384, "noise": {"x": 1}}
    if full:
        j.update(kernel_only={"launch_ms": ms * 0.8, "iters": 7}, strict_batch256={"ms_per_call_median": ms * 0.2, "calls": 9},
                 host_inclusive={"table": {"solve_table_ms": ms * 1.5, "rows": 3}, "single_step": {"ms": 1.0}},
                 other_configs={leg: {"kernel_ms": ms * (k + 2), "solved": 5} for k, leg in enumerate(legs)})
    return j


class Fake:
    """runner and clock: every child takes `seconds`, returns ms[tag][its run number in the phase] (default 10.0) and,
    asked to dump, writes dumps[tag] = {file name: bytes}; the fail_at-th call raises as a child with a non-zero exit does"""

    def __init__(self, ms=None, seconds=10.0, fail_at=0, dumps=None, legs=LEGS):
        self.ms, self.seconds, self.fail_at, self.dumps, self.legs = ms or {}, seconds, fail_at, dumps or {}, legs
        self.calls, self.now, self.dump_dirs = [], 0.0, []

    def clock(self):
        return self.now

    def run(self, build, args, limit):
        full = "--full" in args
        assert limit == (300 if full else 120) and list(args) in (["--full", "--no-cpu-baseline"], [], ["--dump-outputs", *args[1:]])
        n = sum(1 for c in self.calls if c == ("full" if full else "plain", build.tag))
        self.calls.append(("full" if full else "plain", build.tag))
        if len(self.calls) == self.fail_at:
            raise subprocess.CalledProcessError(124, ["timeout"])
        self.now += self.seconds
        if "--dump-outputs" in args:
            d = args[args.index("--dump-outputs") + 1]
            assert os.path.basename(d) == build.tag and n == 0 and not full
            self.dump_dirs.append(d)
            os.makedirs(d)
            for name, data in self.dumps.get(build.tag, {"x.npy": b"same"}).items():
                with open(os.path.join(d, name), "wb") as f:
                    f.write(data)
        return bench_json(self.ms.get(build.tag, [10.0] * (n + 1))[n], full, self.legs)


@pytest.fixture
def libs(tmp_path):
    """library files of three builds (hashed, never loaded) and the tree's own"""
    paths = {}
    for tag in ("p", "a", "b", "tree"):
        paths[tag] = str(tmp_path / f"lib_{tag}.so")
        with open(paths[tag], "wb") as f:
            f.write(tag.encode())
    return paths


def drive(fake, libs, specs, tmp_path, **kw):
    record = str(tmp_path / "record.json")
    status = ab.drive(ab.parse_builds(specs), record, run=fake.run, clock=fake.clock, tree_library=libs["tree"], **kw)
    return status, (json.load(open(record)) if os.path.exists(record) else None)


# ---------------------------------------------------------------- order

def test_order_two_builds_alternate(libs, tmp_path):
    fake = Fake()
    status, rec = drive(fake, libs, [f"p={libs['p']}", "a="], tmp_path, turns=5, phase="plain")
    assert status == 0
    order = [(k // 2, tag) for k, (_, tag) in enumerate(fake.calls)]
    assert order == [(0, "p"), (0, "a"), (1, "a"), (1, "p"), (2, "p"), (2, "a"), (3, "a"), (3, "p"), (4, "p"), (4, "a")]
    assert all(order[2 * t][1] == ("p", "a")[t % 2] for t in range(5))   # each goes first in turns of its own parity
    assert rec["plain"]["turns_completed"] == 5


def test_order_three_builds_rotate(libs, tmp_path):
    fake = Fake()
    drive(fake, libs, [f"p={libs['p']}", f"a={libs['a']}", "b="], tmp_path, turns=5, phase="full")
    tags = [tag for _, tag in fake.calls]
    assert [tags[3 * t:3 * t + 3] for t in range(5)] == [list("pab"), list("abp"), list("bpa"), list("pab"), list("abp")]
    assert ab.rotation(list("pab"), 4) == list("abp") and ab.rotation(list("pa"), 3) == list("ap")


# ---------------------------------------------------------------- verdict

@pytest.mark.parametrize("parent,a,b,want_a,want_b", [
    ([10.0, 11.0], [8.0, 9.0], [12.0, 13.0], (True, False), (False, True)),        # disjoint below, disjoint above
    ([10.0, 11.0], [9.0, 10.5], [10.5, 12.0], (False, False), (False, False)),     # overlapping, either side
    ([10.0, 11.0], [9.0, 10.0], [11.0, 12.0], (False, False), (False, False)),     # touching: max == min, min == max
    ([10.0], [9.0], [11.0], (True, False), (False, True)),                         # single-run lists
    ([10.0], [10.0], [10.0], (False, False), (False, False)),                      # single runs, equal
])
def test_verdict_truth_table(parent, a, b, want_a, want_b):
    v = ab.verdicts({"p": parent, "a": a, "b": b}, "p")
    assert (v["a"]["gain"], v["a"]["loss"]) == want_a and (v["b"]["gain"], v["b"]["loss"]) == want_b
    assert "gain" not in v["p"] and "loss" not in v["p"]
    for tag, runs in (("p", parent), ("a", a), ("b", b)):
        assert v[tag]["runs"] == runs and v[tag]["min"] == min(runs) and v[tag]["max"] == max(runs)


def test_verdicts_reach_the_record(libs, tmp_path):
    fake = Fake(ms={"p": [10.0, 11.0], "a": [8.0, 9.0], "b": [12.0, 10.5]})
    _, rec = drive(fake, libs, [f"p={libs['p']}", f"a={libs['a']}", "b="], tmp_path, turns=2, phase="plain")
    fig = rec["plain"]["figures"]["ms_per_step"]
    assert (fig["a"]["gain"], fig["a"]["loss"], fig["b"]["gain"], fig["b"]["loss"]) == (True, False, False, False)
    assert fig["p"] == {"runs": [10.0, 11.0], "min": 10.0, "max": 11.0}
    assert "slowest" in rec["rule"] and "fastest" in rec["rule"]


# ---------------------------------------------------------------- figures

def test_figures():
    assert ab.figures("plain", bench_json(10.0, False)) == {"ms_per_step": 10.0}
    got = ab.figures("full", bench_json(10.0, True))
    assert set(got) == FULL_NAMES | {f"other_configs.{leg}.kernel_ms" for leg in LEGS}
    assert got["kernel_only.launch_ms"] == 8.0 and got["host_inclusive.table.solve_table_ms"] == 15.0
    assert got["strict_batch256.ms_per_call_median"] == 2.0 and got[f"other_configs.{LEGS[1]}.kernel_ms"] == 30.0
    third = ab.figures("full", bench_json(10.0, True, LEGS + ("cfg9_new_leg",)))
    assert set(third) == set(got) | {"other_configs.cfg9_new_leg.kernel_ms"}


def test_figures_of_both_phases_in_the_record(libs, tmp_path):
    _, rec = drive(Fake(), libs, [f"p={libs['p']}", "a="], tmp_path, turns=2)
    assert set(rec["plain"]["figures"]) == {"ms_per_step"}
    assert set(rec["full"]["figures"]) == FULL_NAMES | {f"other_configs.{leg}.kernel_ms" for leg in LEGS}
    assert rec["plain"]["command"] == "python bench.py" and rec["full"]["command"] == "python bench.py --full --no-cpu-baseline"


# ---------------------------------------------------------------- the first failing child ends the run

@pytest.mark.parametrize("k,plain_turns", [(4, 1), (5, 2), (7, None), (10, None)])
def test_stop_at_first_failing_child(libs, tmp_path, k, plain_turns):
    """two builds, three turns, both phases: calls 1-6 are plain, 7-12 full"""
    fake = Fake(fail_at=k)
    status, rec = drive(fake, libs, [f"p={libs['p']}", "a="], tmp_path, turns=3)
    assert status != 0 and len(fake.calls) == k
    assert fake.dump_dirs and not os.path.exists(os.path.dirname(fake.dump_dirs[0]))
    if plain_turns is not None:   # failed in plain: the record of the last completed turn, and no child of `full`
        assert all(ph == "plain" for ph, _ in fake.calls) and "full" not in rec
        assert rec["plain"]["turns_completed"] == plain_turns
        assert all(len(v["runs"]) == plain_turns for v in rec["plain"]["figures"]["ms_per_step"].values())
    else:                         # failed in full: plain is whole, full holds its completed turns only
        assert rec["plain"]["turns_completed"] == 3
        done = (k - 7) // 2
        assert rec.get("full", {"turns_completed": 0})["turns_completed"] == done
        assert all(len(v["runs"]) == done for fig in rec.get("full", {"figures": {}})["figures"].values() for v in fig.values())


def test_failing_first_child_leaves_no_record(libs, tmp_path):
    fake = Fake(fail_at=1)
    status, rec = drive(fake, libs, [f"p={libs['p']}", "a="], tmp_path, turns=3)
    assert status != 0 and len(fake.calls) == 1 and rec is None


# ---------------------------------------------------------------- budget

@pytest.mark.parametrize("budget,want", [
    (0.0, 5),      # no limit
    (1000.0, 5),   # before turn k: 20 k + 1.2 * 20 = 124 at k = 5 at the most
    (50.0, 2),     # before turn 1: 20 + 24 = 44 <= 50; before turn 2: 40 + 24 = 64 > 50
    (30.0, 1),     # before turn 1: 44 > 30
])
def test_budget(libs, tmp_path, budget, want):
    """a child takes 10 s, so a turn of two builds 20 s"""
    fake = Fake()
    status, rec = drive(fake, libs, [f"p={libs['p']}", "a="], tmp_path, turns=5, phase="plain", budget=budget)
    assert status == 0 and rec["plain"]["turns_completed"] == want and len(fake.calls) == 2 * want
    assert [len(v["runs"]) for v in rec["plain"]["figures"]["ms_per_step"].values()] == [want, want]


def test_budget_has_one_clock_for_both_phases(libs, tmp_path):
    """plain: turns at 0 and 20 s (20 + 24 <= 70).  full: its first turn at 40 s (40 + 0 <= 70), its second would start
    at 60 s: 60 + 24 > 70.  A clock restarted for `full` would have allowed it."""
    fake = Fake()
    _, rec = drive(fake, libs, [f"p={libs['p']}", f"a={libs['a']}", ], tmp_path, turns=2, budget=70.0)
    assert rec["plain"]["turns_completed"] == 2 and rec["full"]["turns_completed"] == 1
    assert all(len(v["runs"]) == 1 for fig in rec["full"]["figures"].values() for v in fig.values())
    assert fake.calls.count(("full", "p")) == fake.calls.count(("full", "a")) == 1


def test_budget_spent_before_a_phase_is_recorded(libs, tmp_path):
    """plain: turns at 0 and 20 s (20 + 24 <= 45).  full would start at 40 s, its longest turn 0 so far: 40 <= 45, one
    turn; under a budget of 35 s plain stops after one turn (44 > 35) and full begins at 20 s: one turn as well; under
    15 s full begins at 20 > 15: no turn, and the record says so."""
    for budget, want in ((45.0, (2, 1)), (35.0, (1, 1)), (15.0, (1, 0))):
        fake = Fake()
        status, rec = drive(fake, libs, [f"p={libs['p']}", "a="], tmp_path, turns=2, budget=budget)
        assert status == 0 and (rec["plain"]["turns_completed"], rec["full"]["turns_completed"]) == want
        assert len(fake.calls) == 2 * sum(want) and (want[1] or rec["full"]["figures"] == {})


def test_budget_uses_the_longest_turn_of_the_current_phase(libs, tmp_path):
    """three builds, 10 s a child: a turn takes 30 s.  Before turn 1: 30 + 36 <= 70; before turn 2: 60 + 36 > 70."""
    fake = Fake()
    _, rec = drive(fake, libs, [f"p={libs['p']}", f"a={libs['a']}", "b="], tmp_path, turns=4, phase="full", budget=70.0)
    assert rec["full"]["turns_completed"] == 2 and len(fake.calls) == 6


# ---------------------------------------------------------------- dumps

@pytest.mark.parametrize("parent,build,want", [
    ({"x.npy": b"abc", "s.npy": b"1"}, {"x.npy": b"abc", "s.npy": b"1"}, {"x.npy": True, "s.npy": True}),    # equal files
    ({"x.npy": b"abc", "s.npy": b"1"}, {"x.npy": b"abd", "s.npy": b"1"}, {"x.npy": False, "s.npy": True}),   # one differing byte
    ({"x.npy": b"abc"}, {"x.npy": b"abc", "s.npy": b"1"}, {"x.npy": True, "s.npy": False}),                  # missing on the parent's side
    ({"x.npy": b"abc", "s.npy": b"1"}, {"x.npy": b"abc"}, {"x.npy": True, "s.npy": False}),                  # missing on the build's side
])
def test_dumps(libs, tmp_path, parent, build, want):
    fake = Fake(dumps={"p": parent, "a": build, "b": parent})
    status, rec = drive(fake, libs, [f"p={libs['p']}", f"a={libs['a']}", "b="], tmp_path, turns=2, phase="plain")
    same = rec["plain"]["dump_outputs_equal_to_parent"]
    assert same["a"] == want and same["b"] == {name: True for name in parent} and "p" not in same
    assert status == (0 if all(want.values()) else 1)
    assert len(fake.dump_dirs) == 3 and not os.path.exists(os.path.dirname(fake.dump_dirs[0]))


# ---------------------------------------------------------------- record merge

def test_record_merge(libs, tmp_path):
    specs = [f"p={libs['p']}", "a=,ACNQP_NO_DIRECT_X=1"]
    _, rec = drive(Fake(), libs, specs, tmp_path, turns=2, phase="plain")
    assert "full" not in rec and rec["builds"] == {
        "p": {"library_sha256": ab.sha256(libs["p"]), "environment": {}},
        "a": {"library_sha256": ab.sha256(libs["tree"]), "environment": {"ACNQP_NO_DIRECT_X": "1"}}}
    plain = rec["plain"]
    _, rec = drive(Fake(), libs, specs, tmp_path, turns=2, phase="full")                  # the same builds: plain is kept
    assert rec["plain"] == plain and rec["full"]["turns_completed"] == 2
    both = rec
    _, rec = drive(Fake(), libs, [specs[0], "a=,ACNQP_NO_DIRECT_X=0"], tmp_path, turns=2, phase="full")   # another pair
    assert "plain" not in rec and rec["builds"]["a"]["environment"] == {"ACNQP_NO_DIRECT_X": "0"}
    with open(tmp_path / "record.json", "w") as f:
        json.dump(both, f)
    with open(libs["p"], "ab") as f:                                                      # another library behind the same path
        f.write(b"!")
    _, rec = drive(Fake(), libs, specs, tmp_path, turns=2, phase="full")
    assert "plain" not in rec and rec["builds"]["p"]["library_sha256"] != both["builds"]["p"]["library_sha256"]
    _, rec = drive(Fake(), libs, specs, tmp_path, turns=1, phase="both")                  # both phases: always a fresh record
    assert rec["plain"]["turns_completed"] == rec["full"]["turns_completed"] == 1


# ---------------------------------------------------------------- a child's environment (the real runner, a stub program)

STUB = """import json, os, sys
print("warming up")
print(json.dumps({"not": "the last one"}))
print(json.dumps({k: v for k, v in os.environ.items() if k.startswith("ACNQP_")}))
print("noise after the JSON line", sys.argv[1:])
sys.exit(%d)
"""


def stub(tmp_path, status=0):
    path = str(tmp_path / "stub_bench.py")
    with open(path, "w") as f:
        f.write(STUB % status)
    return path


def test_child_environment(tmp_path, monkeypatch):
    monkeypatch.setenv("ACNQP_PLAN", "2048,4096")
    monkeypatch.setenv("ACNQP_TRACE", "1")
    monkeypatch.setenv("ACNQP_LIBRARY", "/elsewhere/lib.so")
    x, y = ab.parse_builds(["x=,ACNQP_NO_DIRECT_X=1", "y=/p/lib.so,ACNQP_PLAN=1,2,3"])
    assert ab.run_child(x, ["--full"], 30, program=stub(tmp_path)) == {"ACNQP_NO_DIRECT_X": "1"}
    assert ab.run_child(y, [], 30, program=stub(tmp_path)) == {"ACNQP_PLAN": "1,2,3", "ACNQP_LIBRARY": "/p/lib.so"}
    env = ab.child_env(x, {"PATH": "/bin", "ACNQP_X": "1", "XACNQP_Y": "2"})
    assert env == {"PATH": "/bin", "XACNQP_Y": "2", "ACNQP_NO_DIRECT_X": "1"}


def test_child_that_exits_non_zero_raises(tmp_path):
    (x,) = ab.parse_builds(["x="])
    with pytest.raises(subprocess.CalledProcessError) as e:
        ab.run_child(x, [], 30, program=stub(tmp_path, 3))
    assert e.value.returncode == 3


# ---------------------------------------------------------------- build syntax, command line

def test_build_syntax():
    assert ab.parse_builds(["a="]) == [("a", None, {})]
    assert ab.parse_builds(["a=/p/lib.so"]) == [("a", "/p/lib.so", {})]
    assert ab.parse_builds(["a=,K=V"]) == [("a", None, {"K": "V"})]
    assert ab.parse_builds(["a=/p/lib.so,ACNQP_PLAN=1,2,3,ACNQP_NO_DIRECT_X=1"]) == [("a", "/p/lib.so", {"ACNQP_PLAN": "1,2,3", "ACNQP_NO_DIRECT_X": "1"})]
    assert ab.parse_builds(["a=,ACNQP_PLAN=1,x=2,ACNQP_B=c=d"]) == [("a", None, {"ACNQP_PLAN": "1,x=2", "ACNQP_B": "c=d"})]   # lower case: no new pair
    assert ab.parse_builds(["a=rel/lib.so"])[0].lib == os.path.abspath("rel/lib.so")
    assert [b.tag for b in ab.parse_builds(["p=", "a=", "b=/l.so"])] == ["p", "a", "b"]
    for bad in (["a=", "a=/p/lib.so"], ["a"], ["=lib.so"]):   # a duplicate tag, a missing `=`, no tag
        with pytest.raises(ValueError):
            ab.parse_builds(bad)


def test_command_line(libs, tmp_path, monkeypatch):
    for bad in (["p=", "a"], ["p=", "p="], ["p="], ["p=", "a=", "b="]):   # ... and --record is required beyond one build
        with pytest.raises(SystemExit) as e:
            ab.main(bad, run=None)
        assert e.value.code == 2
    seen = {}
    monkeypatch.setattr(ab, "drive", lambda builds, record, *a, **kw: seen.update(builds=builds, record=record, a=a) or 0)
    assert ab.main(["p=/p.so", "a=", "--turns", "3", "--phase", "full", "--budget", "60"]) == 0
    assert seen["record"] == os.path.join(ROOT, "profiles", "bench_ab.json") and seen["a"] == (3, "full", 60.0)
    assert ab.main(["--record", "r.json", "p=", "a=", "b=,ACNQP_PLAN=1,2"]) == 0
    assert seen["record"] == "r.json" and seen["builds"][2] == ("b", None, {"ACNQP_PLAN": "1,2"})
