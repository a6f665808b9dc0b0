"""``polish_kernel<4 | 8>`` (adacharge_amd/csrc/acn_qp_polish.hpp) held to its specification oracle/polish_ref.py, problem by
problem, on the cases of tests/polish_cases.py (tests/test_polish_cases.py proves them fit on the CPU).

Every case is padded to every shape (t_max in own, 13, 16, 17, 29, 32; K in own, 4) whose route runs the polish, and
launched four times per shape through the device entry with poisoned outputs:
  hand    max_iter = P, retry_passes = 0, polish_iters = 0   -- the hand-over point (x, and y in the caller's units)
  pol     polish_iters = P, retry_passes = 0                 -- the polished run
  ref     polish_iters = 0, retry_passes = 0                 -- the ADMM alone
  only    pol with eps_abs = eps_rel = 1e-30                 -- a launch in which nothing but the polish can end SOLVED
A problem the polish gives up on is resumed from the hand-over point and may end SOLVED a few checks later, inside the 96
iterations a polish may add: ``iters`` alone does not tell the two apart (the N = 3 case: six of 24 on one route).  So WHO
WAS POLISHED is read from ``only``: the residual test never passes there, the iterate at P is the same (asserted: the
polished problems have the bits of ``pol``), and SOLVED means the polish accepted.
The specification then starts from the DEVICE's hand-over point of each shape (equal points are run once).  A problem is
handed over when ``hand`` leaves it MAX_ITER or SOLVED_INACCURATE (an infeasibility certified before P ends the problem in
the solver kernel) and its multipliers do not count more rows than the row tables hold (polish_cases.declined_rows).
``ref`` runs without retry passes like ``pol``, so that a declined problem can be held to its bits.

Last, two wave-route cases in a fresh child process per setting: the launch alongside and ACNQP_NO_POLISH_ALONGSIDE=1 give
the same bits at an early hand-over (tests/test_polish_alongside_gpu.py holds that at P = 300 / 400)."""
import collections
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests import polish_cases as PC

CASES = list(PC.CASES)
POLISH_FAMILIES = {"wave1", "wave2", "wave3", "wave4", "tiled_ct1", "tiled_ct2", "long_lds"}   # acn_qp_route.hpp: on chip, N <= 64, T <= 32
COUNTERS = ("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt")
WHY = {"rows": "gave_up_rows", "pivot": "gave_up_pivot", "rounds": "gave_up_rounds", "verify": "gave_up_kkt"}
X_TOL = 1e-7      # A: the constant of test_polish_agrees_with_its_numpy_specification; the specification's own spread is 2e-11
Y_REL = 2e-3      # the least-norm multipliers of a regularised, nearly singular system agree to three digits (same test)
# pri_res / dua_res of a polished problem against the specification's primal / stat, in units of the acceptance limits of
# the final check (1e-8 and 1e-8 max(1, |q|_inf)): 10x the worst measured on an MI355X [in brackets]
RES_TOL = {"pri": 4.4e-5, "dua": 1.8e-5}   # [4.36e-6 (n64_lin_t16_peak@100), 1.73e-6 (jpl_soc_t12_one@200)]


@functools.lru_cache(maxsize=None)
def _ran(case):
    from adacharge_amd.backend import SiteHandle, default_options

    name, P, _, _ = PC.CASES[case]
    pool = PC.pool(name)
    h = SiteHandle(pool.site, 0)
    runs = []
    for t in sorted({pool.Tm} | {t for t in PC.T_PADS if t >= pool.Tm}):
        for k in sorted({pool.K} | {k for k in PC.K_PADS if k >= pool.K}):
            fam, pol = h.route(t, k, pool.B)
            tables = PC.polish_tables(pool.site, t, k, fam.startswith("tiled"))
            if not pol:
                continue
            assert tables[2] >= 0, (case, fam, t, k, tables)   # the restated LDS tables agree that a polish fits this shape
            padded = H.pad_batch(pool, t, k)
            hand = H.launch_poisoned(h, padded, default_options(max_iter=P, retry_passes=0, polish_iters=0))
            s0 = h.polish_stats()
            out = H.launch_poisoned(h, padded, default_options(polish_iters=P, retry_passes=0))
            s1 = h.polish_stats()
            ref = H.launch_poisoned(h, padded, default_options(polish_iters=0, retry_passes=0))
            only = H.launch_poisoned(h, padded, default_options(polish_iters=P, retry_passes=0, eps_abs=1e-30, eps_rel=1e-30, max_iter=P + 20))
            open_ = [int(b) for b in np.flatnonzero(np.isin(hand["status"], (2, 5)))]
            declined = [b for b in open_ if PC.declined_rows(pool, b, hand["y"][b], t)[1]]
            runs.append(dict(shape=(t, k), fam=fam, tables=tables, padded=padded, hand=hand, pol=out, ref=ref, only=only, stats={c: s1[c] - s0[c] for c in COUNTERS},
                             declined=declined, handed=[b for b in open_ if b not in declined]))
    h.close()
    res = iter(PC.spec_many([PC.spec_args(pool, b, r["hand"]["x"][b], r["hand"]["y"][b]) for r in runs for b in r["handed"]]))
    for r in runs:
        r["spec"] = {b: next(res) for b in r["handed"]}
        # what the kernel owes at this shape: the specification's verdict and reason, but `rows` where a round of the problem
        # outgrows the LDS tables the padded shape leaves (polish_cases.polish_tables; the specification has no such limit)
        r["owed"] = {b: ("rows" if PC.outgrows(info, r["tables"]) else "accept" if info["ok"] else info["why"]) for b, (_, info) in r["spec"].items()}
        r["polished"] = [b for b in r["handed"] if r["only"]["status"][b] == 1]
    return pool, runs


def _where(case, r):
    return f"{case} on {r['fam']} (t_max {r['shape'][0]}, K {r['shape'][1]})"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_who_was_polished_is_known_not_guessed(case):
    pool, runs = _ran(case)
    assert runs, case
    for r in runs:
        print(f"[polish] {_where(case, r)}: handed {len(r['handed'])}, declined {r['declined']}, polished {len(r['polished'])}, {r['stats']}")
        for key in ("x", "y", "pri_res", "dua_res", "obj"):
            for run in ("hand", "pol", "ref"):
                assert not np.isnan(r[run][key]).any(), f"{_where(case, r)}: {run} {key} left unwritten"
        assert (r["hand"]["iters"][r["handed"]] == PC.CASES[case][1]).all(), (_where(case, r), r["hand"]["iters"])
        assert r["stats"]["attempted"] == len(r["handed"]), (_where(case, r), r["stats"], r["handed"], r["declined"])
        assert r["stats"]["solved"] == len(r["polished"]), (_where(case, r), r["stats"], r["polished"])
        for b in r["polished"]:   # SOLVED within the window, with the bits of the launch in which only the polish solves
            assert r["pol"]["status"][b] == 1 and 0 < r["pol"]["iters"][b] - r["hand"]["iters"][b] <= PC.WINDOW, (_where(case, r), b, r["pol"]["iters"][b])
            for key in ("x", "y", "iters", "pri_res", "dua_res", "obj"):
                assert np.array_equal(r["pol"][key][b], r["only"][key][b]), (_where(case, r), b, key)
        assert sum(r["stats"][c] for c in COUNTERS[1:]) == r["stats"]["attempted"], (_where(case, r), r["stats"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_the_kernel_polishes_exactly_what_the_specification_accepts(case):
    pool, runs = _ran(case)
    fragile = set(PC.ROUND_FRAGILE.get(case, ()))
    for r in runs:
        accepted = {b for b, w in r["owed"].items() if w == "accept"}
        odd = accepted ^ set(r["polished"])
        why = collections.Counter(w for w in r["owed"].values() if w != "accept")
        moved = sorted(b for b, (_, info) in r["spec"].items() if PC.outgrows(info, r["tables"]))
        print(f"[polish] {_where(case, r)}: owed: accept {len(accepted)}, give up {dict(why)} (outgrow the LDS tables {r['tables']}: {moved}); "
              f"kernel {r['stats']}; disagree {sorted(odd)}")
        assert odd <= fragile and len(odd) <= 2, (_where(case, r), sorted(odd), {b: r["spec"][b][1] for b in odd})
        for reason, counter in WHY.items():
            assert abs(r["stats"][counter] - why.get(reason, 0)) <= len(odd), (_where(case, r), reason, r["stats"], dict(why))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_polished_answers_are_the_specifications(case):
    pool, runs = _ran(case)
    worst = dict(x=0.0, y=0.0, pri=0.0, dua=0.0)
    for r in runs:
        out, padded = r["pol"], r["padded"]
        for b in r["polished"]:
            xs, info = r["spec"][b]
            if r["owed"][b] != "accept":
                continue
            T = xs.shape[1]
            x, y = out["x"][b], out["y"][b]
            assert not x[:, T:].any() and not y[:, T:].any(), (_where(case, r), b)
            qn = max(1.0, float(np.abs(pool.q[b]).max()))
            d = dict(x=float(np.abs(x[:, :T] - xs).max()),
                     y=float(np.abs(y[:, :T] - info["y"]).max()) / max(1.0, float(np.abs(info["y"]).max())),
                     pri=abs(float(out["pri_res"][b]) - max(info["primal"], 0.0)) / 1e-8,
                     dua=abs(float(out["dua_res"][b]) - info["stat"]) / (1e-8 * qn))
            worst = {k: max(worst[k], v) for k, v in d.items()}
            assert d["x"] <= X_TOL and d["y"] <= Y_REL, (_where(case, r), b, d)
            assert d["pri"] <= RES_TOL["pri"] and d["dua"] <= RES_TOL["dua"], (_where(case, r), b, d)
            obj = out["obj"][b] + kkt.prox_terms(padded, b, x)
            bad = kkt.failures(kkt.certify(padded, b, x, y, obj), 1)
            assert not bad, (_where(case, r), b, bad)
    print(f"[polish] {case}: worst |x - x_spec| {worst['x']:.2e} A, y {worst['y']:.2e} relative, pri_res {worst['pri']:.2e} and dua_res "
          f"{worst['dua']:.2e} of the check's limits")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_one_problem_one_polished_answer_whatever_the_padding(case):
    pool, runs = _ran(case)
    worst = 0.0
    for b in range(pool.B):
        T = int(pool.T[b])
        xs = [(r, r["pol"]["x"][b][:, :T]) for r in runs if b in r["polished"]]
        for r, x in xs[1:]:
            d = float(np.abs(x - xs[0][1]).max())
            worst = max(worst, d)
            assert d <= X_TOL, (_where(case, r), _where(case, xs[0][0]), b, d)
    print(f"[polish] {case}: worst polished |x - x'| across {len(runs)} padded shapes {worst:.2e} A")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_newton_rounds_are_the_specifications_on_a_late_hand_over(case):
    """iters - P: the instrument for the data the solver kernels publish at the hand-over -- a mis-scaled y costs rounds"""
    pool, runs = _ran(case)
    late = PC.CASES[case][3]
    fragile = set(PC.ROUND_FRAGILE.get(case, ()))
    for r in runs:
        diff = {b: int(r["pol"]["iters"][b] - r["hand"]["iters"][b]) - r["spec"][b][1]["rounds"] for b in r["polished"] if r["spec"][b][1]["ok"]}
        firm = {b: d for b, d in diff.items() if b not in fragile}
        print(f"[polish] {_where(case, r)}: rounds kernel - specification, firm {sorted(collections.Counter(firm.values()).items())}, "
              f"fragile {sorted(collections.Counter(d for b, d in diff.items() if b in fragile).items())}")
        if late:
            assert not any(firm.values()), (_where(case, r), {b: d for b, d in firm.items() if d})


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_give_ups_leave_no_trace(case):
    name = PC.CASES[case][0]
    pool, runs = _ran(case)
    twin = PC.twin(name)["status"]
    # a disc of radius zero (the N = 3 site's pod row: three balanced phases, limit 2e-15 A) pins its currents to the apex,
    # where every direction is normal to it: the certificate's alignment of y with u / |u| says nothing there (|u| = 1e-16)
    apex = int(pool.site.cone) == 1 and bool((np.asarray(pool.site.limits, float) < 1e-9).any())
    for r in runs:
        out, ref, padded = r["pol"], r["ref"], r["padded"]
        for b in r["declined"]:   # no hand-over happened: the bits of the run without a polish
            for key in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj"):
                assert np.array_equal(out[key][b], ref[key][b]), (_where(case, r), b, key)
        for b in r["declined"] + [b for b in r["handed"] if b not in r["polished"]]:
            st = int(out["status"][b])
            assert st == int(twin[b]), (_where(case, r), b, st, int(twin[b]), int(out["iters"][b]))
            T = int(pool.T[b])
            assert not out["x"][b][:, T:].any() and not out["y"][b][:, T:].any(), (_where(case, r), b)
            obj = out["obj"][b] + kkt.prox_terms(padded, b, out["x"][b])
            bad = kkt.failures(kkt.certify(padded, b, out["x"][b], out["y"][b], obj), st)
            if apex:
                bad.pop("cone", None)
            assert not bad, (_where(case, r), b, st, bad)


@pytest.mark.gpu
def test_cases_reach_every_family_shape_and_give_up_reason_on_the_device():
    """accepted answers (equal to the specification's: the tests above) from every family that runs the polish, from both
    instantiations at TQ = 4, 5 and 8 with a short last quarter, with LINEAR rows, a tight peak row, equalities, K = 4 and
    lb > 0; and every give-up reason the cases are built for"""
    fams, tq, kinds, gave = set(), set(), set(), collections.Counter()
    for case in CASES:
        pool, runs = _ran(case)
        site = pool.site
        for r in runs:
            t, k = r["shape"]
            gave.update({c: r["stats"][c] for c in COUNTERS[2:]})
            gave["declined"] += len(r["declined"])
            gave["outgrown"] += sum(w == "rows" and r["spec"][b][1]["why"] != "rows" for b, w in r["owed"].items())
            # an infeasible problem that the DEVICE had not certified at P: handed over, given up on, resumed to status 3
            twin = PC.twin(PC.CASES[case][0])["status"]
            gave["infeasible"] += sum(twin[b] == 3 and r["pol"]["status"][b] == 3 for b in r["handed"] if b not in r["polished"])
            for b in r["polished"]:
                if r["owed"][b] != "accept":
                    continue
                kinds.add(f"N{pool.N}")
                fams.add(r["fam"])
                tq.add((8 if t > 16 else 4, (t + 3) >> 2, t % 4 != 0))
                T = int(pool.T[b])
                kinds.add("soc" if int(site.cone) == 1 else "linear")
                if site.has_peak and np.abs(r["pol"]["y"][b][site.Mg - 1]).max() > 0:
                    kinds.add("scalar_peak" if np.ptp(pool.peak[b][:T]) == 0 else "vector_peak")
                kinds.add("eq" if pool.s_eq[b] else "ineq")
                if pool.K == 4 and pool.s_len[b, 3].any():
                    kinds.add("four_sessions")
                if k == 4 and pool.K < 4:
                    kinds.add("padded_slots")
                if (pool.lb[b] > 0).any():
                    kinds.add("lb_positive")
    print(f"[polish] families {sorted(fams)}, (instantiation, TQ, short quarter) {sorted(tq)}, {sorted(kinds)}, give-ups {dict(gave)}")
    assert fams == POLISH_FAMILIES, sorted(POLISH_FAMILIES ^ fams)
    assert {(4, 4, True), (4, 4, False), (8, 5, True), (8, 8, True), (8, 8, False)} <= tq, sorted(tq)
    assert {"soc", "linear", "scalar_peak", "vector_peak", "eq", "ineq", "four_sessions", "padded_slots", "lb_positive"} <= kinds, sorted(kinds)
    assert {"N3", "N8", "N52", "N54", "N64"} <= kinds, sorted(kinds)
    assert gave["declined"] and gave["gave_up_rounds"] and gave["gave_up_kkt"] and gave["outgrown"] and gave["infeasible"] >= 3, dict(gave)


@functools.lru_cache(maxsize=None)
def _children(case, t_max, k):
    """the polished launch of a case in a fresh child process per setting (the switch is read once per process)"""
    import os
    import subprocess
    import sys
    import tempfile

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env in (("on", {}), ("off", {"ACNQP_NO_POLISH_ALONGSIDE": "1"})):
            f = os.path.join(tmp, tag + ".npz")
            e = {key: v for key, v in os.environ.items() if not key.startswith("ACNQP_")}
            subprocess.run([sys.executable, PC.__file__, "--solve", case, str(t_max), str(k), f], check=True, env=dict(e, **env), timeout=300)
            with np.load(f) as z:
                out[tag] = {key: z[key] for key in z.files}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case,t_max,k", [("ct54_soc_peak_one@20", 13, 1), ("n8_soc@40", 5, 1)])
def test_alongside_and_serial_give_the_same_bits_at_an_early_hand_over(case, t_max, k):
    """wave routes on which the launch alongside is issued (wave4 and wave1; not the two-row-tile route of horizons <= 12),
    most of the batch handed over at 20 / 40 iterations while the rest still runs: with the launch alongside and with
    ACNQP_NO_POLISH_ALONGSIDE=1 the same bits, and those of this process's own polished launch"""
    runs = _children(case, t_max, k)
    on, off = runs["on"], runs["off"]
    print(f"[polish] {case} on {on['family']} (t_max {t_max}, K {k}): handed over {int(on['attempted'])}, polished {int(on['solved'])}, "
          f"taken alongside {int(on['alongside'])} / {int(off['alongside'])}")
    assert str(on["family"]) in ("wave1", "wave2", "wave4") and str(off["family"]) == str(on["family"])
    assert int(on["attempted"]) >= 8 and int(on["solved"]) >= 8
    assert int(on["alongside"]) > 0 and int(off["alongside"]) == 0   # (measured: all 20 and all 24 taken alongside)
    assert (int(on["attempted"]), int(on["solved"])) == (int(off["attempted"]), int(off["solved"]))
    own = next(r for r in _ran(case)[1] if r["shape"] == (t_max, k))["pol"]
    for key in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj"):
        assert np.array_equal(on[key], off[key]), (case, key)
        assert np.array_equal(on[key], own[key]), (case, key, "child against this process")
