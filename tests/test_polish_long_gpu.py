"""``polish_long_kernel`` (adacharge_amd/csrc/acn_qp_polish_long.hpp: horizons 33 ... 288, N <= 64) held to the polish's
specification oracle/polish_ref.py, problem by problem, on the cases of tests/polish_long_cases.py (tests/test_polish_long_cases.py
proves them fit on the CPU).  Follows tests/test_polish_gpu.py: every case at every padded shape gets four launches with
poisoned outputs on a ``polish_long=True`` handle,
  hand    max_iter = P, retry_passes = 0, polish_iters = 0   -- the hand-over point (x, and y in the caller's units)
  pol     polish_iters = P, retry_passes = 0                 -- the polished run
  ref     polish_iters = 0, retry_passes = 0                 -- the ADMM alone
  only    pol with eps_abs = eps_rel = 1e-30                 -- a launch in which nothing but the polish can end SOLVED
WHO WAS POLISHED is read from ``only``; the specification starts from the DEVICE's hand-over point of each shape, with its
MAX_ROWS raised to the worst case of the shape (polish_long_cases.spec_many).  The long kernel's tables hold that worst
case: every open problem is handed over, and none is given up for `rows`."""
import collections
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests import polish_cases as PC
from tests import polish_long_cases as LC

CASES = list(LC.CASES)
LONG_FAMILIES = {"wave5", "long_ws"}   # acn_qp_route.hpp: polish_long_shape
COUNTERS = ("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt")
WHY = {"rows": "gave_up_rows", "pivot": "gave_up_pivot", "rounds": "gave_up_rounds", "verify": "gave_up_kkt"}
X_TOL = 1e-7      # A   (tests/test_polish_gpu.py's constants)
Y_REL = 2e-3
# pri_res / dua_res of a polished problem against the specification's primal / stat, in units of the acceptance limits of the
# final check (1e-8 and 1e-8 max(1, |q|_inf)): 10x the worst measured on an MI355X [in brackets]
RES_TOL = {"pri": 1.3e-5, "dua": 6.1e-6}   # [1.24e-6 (n8_t288@100), 6.05e-7 (n8_t144@100)]
# problems on which the kernel and the specification may disagree about acceptance, with the reason (at most two per case)
DISAGREE = {}
RATE_TOL = 1e-4 * 32   # the project's parity bound (tests/test_gpu_parity.py)


@functools.lru_cache(maxsize=None)
def _ran(case):
    from adacharge_amd.backend import SiteHandle, default_options

    name, P = LC.CASES[case][:2]
    pool = LC.pool(name)
    h = SiteHandle(pool.site, 0, polish_long=True)
    runs = []
    for t, k in LC.shapes(case):
        fam, pol = h.route(t, k, pool.B)
        assert pol == 1 and fam in LONG_FAMILIES, (case, t, k, fam, pol)
        padded = H.pad_batch(pool, t, k)
        hand = H.launch_poisoned(h, padded, default_options(max_iter=P, retry_passes=0, polish_iters=0))
        s0 = h.polish_stats()
        out = H.launch_poisoned(h, padded, default_options(polish_iters=P, retry_passes=0))
        s1 = h.polish_stats()
        ref = H.launch_poisoned(h, padded, default_options(polish_iters=0, retry_passes=0))
        only = H.launch_poisoned(h, padded, default_options(polish_iters=P, retry_passes=0, eps_abs=1e-30, eps_rel=1e-30, max_iter=P + 20))
        handed = [int(b) for b in np.flatnonzero(np.isin(hand["status"], (2, 5)))]
        runs.append(dict(shape=(t, k), fam=fam, padded=padded, hand=hand, pol=out, ref=ref, only=only, stats={c: s1[c] - s0[c] for c in COUNTERS},
                         handed=handed))
    h.close()
    res = iter(LC.spec_many([(LC.worst_rows(pool.site, r["shape"][0]), PC.spec_args(pool, b, r["hand"]["x"][b], r["hand"]["y"][b]))
                             for r in runs for b in r["handed"]]))
    for r in runs:
        r["spec"] = {b: next(res) for b in r["handed"]}
        r["owed"] = {b: ("accept" if info["ok"] else info["why"]) for b, (_, info) in r["spec"].items()}
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
        print(f"[polish-long] {_where(case, r)}: handed {len(r['handed'])}, polished {len(r['polished'])}, {r['stats']}")
        for key in ("x", "y", "pri_res", "dua_res", "obj"):
            for run in ("hand", "pol", "ref"):
                assert not np.isnan(r[run][key]).any(), f"{_where(case, r)}: {run} {key} left unwritten"
        assert r["handed"] and (r["hand"]["iters"][r["handed"]] == LC.CASES[case][1]).all(), (_where(case, r), r["hand"]["iters"])
        assert r["stats"]["attempted"] == len(r["handed"]), (_where(case, r), r["stats"], r["handed"])
        assert r["stats"]["solved"] == len(r["polished"]), (_where(case, r), r["stats"], r["polished"])
        assert r["stats"]["gave_up_rows"] == 0, (_where(case, r), r["stats"])
        for b in r["polished"]:   # SOLVED within the window, with the bits of the launch in which only the polish solves
            assert r["pol"]["status"][b] == 1 and 0 < r["pol"]["iters"][b] - r["hand"]["iters"][b] <= LC.WINDOW, (_where(case, r), b, r["pol"]["iters"][b])
            for key in ("x", "y", "iters", "pri_res", "dua_res", "obj"):
                assert np.array_equal(r["pol"][key][b], r["only"][key][b]), (_where(case, r), b, key)
        assert sum(r["stats"][c] for c in COUNTERS[1:]) == r["stats"]["attempted"], (_where(case, r), r["stats"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_the_kernel_polishes_exactly_what_the_specification_accepts(case):
    pool, runs = _ran(case)
    allowed = set(DISAGREE.get(case, {}))
    for r in runs:
        accepted = {b for b, w in r["owed"].items() if w == "accept"}
        odd = accepted ^ set(r["polished"])
        why = collections.Counter(w for w in r["owed"].values() if w != "accept")
        print(f"[polish-long] {_where(case, r)}: owed: accept {len(accepted)}, give up {dict(why)}; kernel {r['stats']}; disagree {sorted(odd)}")
        assert odd <= allowed and len(odd) <= 2, (_where(case, r), sorted(odd), {b: r["spec"][b][1] for b in odd})
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
            print(f"[polish-long] {_where(case, r)} problem {b}: {d}")
            assert d["x"] <= X_TOL and d["y"] <= Y_REL, (_where(case, r), b, d)
            assert d["pri"] <= RES_TOL["pri"] and d["dua"] <= RES_TOL["dua"], (_where(case, r), b, d)
            obj = out["obj"][b] + kkt.prox_terms(padded, b, x)
            bad = kkt.failures(kkt.certify(padded, b, x, y, obj), 1)
            assert not bad, (_where(case, r), b, bad)
    print(f"[polish-long] {case}: worst |x - x_spec| {worst['x']:.2e} A, y {worst['y']:.2e} relative, pri_res {worst['pri']:.2e} and dua_res "
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
    print(f"[polish-long] {case}: worst polished |x - x'| across {len(runs)} padded shapes {worst:.2e} A")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if LC.CASES[c][3]])
def test_newton_rounds_are_the_specifications_on_a_late_hand_over(case):
    """iters - P: the instrument for the data the solver kernels publish at the hand-over -- a mis-scaled y costs rounds"""
    pool, runs = _ran(case)
    for r in runs:
        diff = {b: int(r["pol"]["iters"][b] - r["hand"]["iters"][b]) - r["spec"][b][1]["rounds"] for b in r["polished"] if r["spec"][b][1]["ok"]}
        print(f"[polish-long] {_where(case, r)}: rounds kernel - specification {sorted(collections.Counter(diff.values()).items())}")
        assert diff and not any(diff.values()), (_where(case, r), {b: d for b, d in diff.items() if d})


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_give_ups_leave_no_trace(case):
    name = LC.CASES[case][0]
    pool, runs = _ran(case)
    twin = LC.twin(name)["status"]
    for r in runs:
        out, padded = r["pol"], r["padded"]
        for b in [b for b in r["handed"] if b not in r["polished"]]:
            st = int(out["status"][b])
            assert st == int(twin[b]), (_where(case, r), b, st, int(twin[b]), int(out["iters"][b]))
            T = int(pool.T[b])
            assert not out["x"][b][:, T:].any() and not out["y"][b][:, T:].any(), (_where(case, r), b)
            obj = out["obj"][b] + kkt.prox_terms(padded, b, out["x"][b])
            bad = kkt.failures(kkt.certify(padded, b, out["x"][b], out["y"][b], obj), st)
            assert not bad, (_where(case, r), b, st, bad)


@pytest.mark.gpu
def test_cases_reach_both_families_cones_a_tight_peak_four_sessions_and_period_256():
    fams, kinds, gave = set(), set(), collections.Counter()
    for case in CASES:
        pool, runs = _ran(case)
        site = pool.site
        for r in runs:
            gave.update({c: r["stats"][c] for c in COUNTERS[2:]})
            for b in r["polished"]:
                if r["owed"][b] != "accept":
                    continue
                fams.add(r["fam"])
                T = int(pool.T[b])
                kinds.add("soc" if int(site.cone) == 1 else "linear")
                if site.has_peak and np.abs(r["pol"]["y"][b][site.Mg - 1]).max() > 0:
                    kinds.add("tight_peak")
                if pool.K == 4 and pool.s_len[b, 3].any():
                    kinds.add("four_sessions")
                if T > 256 and np.abs(r["pol"]["x"][b][:, 256:T]).max() > 0:
                    kinds.add("period_256")
    print(f"[polish-long] families {sorted(fams)}, {sorted(kinds)}, give-ups {dict(gave)}")
    assert fams == LONG_FAMILIES, sorted(LONG_FAMILIES ^ fams)
    assert {"soc", "linear", "tight_peak", "four_sessions", "period_256"} <= kinds, sorted(kinds)
    assert gave["gave_up_rounds"] and not gave["gave_up_rows"], dict(gave)


@pytest.mark.gpu
def test_same_bits_alone_and_in_a_batch_three_times_the_size():
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import ProblemBatch

    case = "ct54_t48@40"
    name, P = LC.CASES[case][:2]
    pool = LC.pool(name)
    h = SiteHandle(pool.site, 0, polish_long=True)
    o = default_options(polish_iters=P, retry_passes=0)
    alone = H.launch_poisoned(h, pool, o)
    s0 = h.polish_stats()
    three = H.launch_poisoned(h, ProblemBatch.concatenate([pool, pool, pool]), o)
    s1 = h.polish_stats()
    h.close()
    assert s1["attempted"] - s0["attempted"] >= 3 * 2 and s1["solved"] - s0["solved"] >= 3 * 2, (s0, s1)
    for key in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj"):
        for part in range(3):
            assert np.array_equal(three[key][part * pool.B:(part + 1) * pool.B], alone[key]), (key, part)


KEYS = ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")


def _launch(h, batch, options, want_y=True):
    """H.launch_poisoned with or without the caller's multiplier array (without: the launch keeps them in its own scratch)"""
    import torch

    from adacharge_amd.backend import DeviceBatch

    if want_y:
        return H.launch_poisoned(h, batch, options)
    dev = DeviceBatch(batch, "cuda:0", want_y=False)
    for a in (dev.x, dev.pri_res, dev.dua_res, dev.obj):
        a.fill_(float("nan"))
    dev.iters.fill_(-1)
    dev.status.fill_(-1)
    h.solve_device(dev, options, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: getattr(dev, k).cpu().numpy() for k in KEYS if k != "y"}


def _in_turn_on_one_handle_and_each_on_a_fresh_one(site, launches, **switch):
    """[(batch, options, want_y)] launched in turn on ONE handle and one stream -- the stream's scratch buffer
    (acn_qp_polplan.hpp: PolishScratch) is carved anew for each -- against the same launch on a handle of its own: the bits"""
    from adacharge_amd.backend import SiteHandle

    h = SiteHandle(site, 0, **switch)
    for n, (batch, o, want_y) in enumerate(launches):
        s0 = h.polish_stats()
        got = _launch(h, batch, o, want_y)
        rose = h.polish_stats()["attempted"] - s0["attempted"]
        fresh = SiteHandle(site, 0, **switch)
        ref = _launch(fresh, batch, o, want_y)
        fresh.close()
        print(f"[polish-plan] launch {n}: {batch.B} x {batch.N} x {batch.Tm} (K {batch.K}), multipliers {'wanted' if want_y else 'not wanted'}: "
              f"{rose} handed to the polish, status {got['status'].tolist()}")
        assert rose > 0, (n, rose)   # (the condition that this launch tests anything)
        assert set(got) == set(KEYS) - (set() if want_y else {"y"})
        for key in got:
            assert np.array_equal(got[key], ref[key]), (n, key)
    h.close()


@pytest.mark.gpu
def test_one_scratch_buffer_serves_the_on_chip_and_the_long_kind_in_turn():
    from adacharge_amd.backend import SiteHandle, default_options

    short_name, short_P = "ct54_soc_two", 40          # caltech54 SOC at horizon 12, K = 2: the on-chip polish
    at = PC.twin(short_name, short_P)                  # (the CPU twin at P, as polish_cases.cpu_case asks it)
    still_open = [int(b) for b in np.flatnonzero(at["status"] != 1)][:8]
    assert still_open, at["status"]
    short = PC.pool(short_name).subset(still_open)
    long_name, long_P = LC.CASES["ct54_t48@40"][:2]    # the same site at horizon 48: the long-horizon polish
    lng = LC.pool(long_name)
    assert short.B <= 8 and lng.B <= 8 and short.Tm == 12
    h = SiteHandle(lng.site, 0, polish_long=True)
    fams = [h.route(b.Tm, b.K, b.B) for b in (short, lng)]
    h.close()
    assert fams[0][1] == 1 and fams[0][0] not in LONG_FAMILIES and fams[1][1] == 1 and fams[1][0] in LONG_FAMILIES, fams
    a = (short, default_options(polish_iters=short_P, retry_passes=0), True)
    b = (lng, default_options(polish_iters=long_P, retry_passes=0), True)
    _in_turn_on_one_handle_and_each_on_a_fresh_one(lng.site, [a, b, a, b], polish_long=True)


@pytest.mark.gpu
def test_one_scratch_buffer_serves_the_wide_kind_with_and_without_the_callers_multipliers():
    from adacharge_amd.backend import default_options
    from tests import polish_wide_cases as WC

    case = "n65_soc"   # the smallest site of tests/polish_wide_cases.py, six problems
    pool = WC.pool(WC.CASES[case][0])
    o = default_options(**WC.start_options(case))
    _in_turn_on_one_handle_and_each_on_a_fresh_one(pool.site, [(pool, o, True), (pool, o, False), (pool, o, True)], polish_wide=True)


@pytest.mark.gpu
def test_the_switch_is_off_by_default_and_leaves_short_horizons_alone():
    from adacharge_amd.backend import SiteHandle, default_options

    case = "ct54_t48@40"
    name, P = LC.CASES[case][:2]
    pool = LC.pool(name)
    off, on = SiteHandle(pool.site, 0), SiteHandle(pool.site, 0, polish_long=True)
    for t, k in LC.shapes(case):
        assert off.route(t, k, pool.B)[1] == 0 and on.route(t, k, pool.B)[1] == 1, (t, k)
        assert off.route(t, k, pool.B)[0] == on.route(t, k, pool.B)[0]
    s0 = off.polish_stats()
    plain = H.launch_poisoned(off, pool, default_options(polish_iters=P, retry_passes=0))
    ref = H.launch_poisoned(off, pool, default_options(polish_iters=0, retry_passes=0))
    assert off.polish_stats()["attempted"] == s0["attempted"]
    for key in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj"):   # off: polish_iters means nothing on these shapes
        assert np.array_equal(plain[key], ref[key]), key
    off.close()
    on.close()
    # a t_max <= 32 case of tests/polish_cases.py: the bits of a plain handle
    short_case = "ct54_soc_t24_peak@100"
    sname, sP = PC.CASES[short_case][:2]
    spool = PC.pool(sname)
    off, on = SiteHandle(spool.site, 0), SiteHandle(spool.site, 0, polish_long=True)
    assert off.route(spool.Tm, spool.K, spool.B) == on.route(spool.Tm, spool.K, spool.B) and on.route(spool.Tm, spool.K, spool.B)[1] == 1
    o = default_options(polish_iters=sP, retry_passes=0)
    a, b = H.launch_poisoned(off, spool, o), H.launch_poisoned(on, spool, o)
    assert on.polish_stats()["attempted"] > 0
    off.close()
    on.close()
    for key in ("x", "y", "status", "iters", "pri_res", "dua_res", "obj"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.gpu
def test_through_the_public_surface_a_horizon_36_snapshot_ends_at_the_certified_optimum():
    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, quick_charge, sites, total_energy
    from adacharge_amd.acn import Interface
    from oracle.ipm import solve_certified
    from oracle.ref_problem import build_reference_problem

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3), ObjectiveComponent(total_energy, 0.5)]
    spec = [("quick_charge", 1, {}), ("equal_share", 1e-3, {}), ("total_energy", 0.5, {})]
    sl = sites.random_sessions_general(infra, 36, np.random.default_rng(75), two_per_evse=False, min_rates=True, demand_scale=1.5)
    plain = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", solver_options={"polish_iters": 40})
    plain.solve(sl, infra)
    opt = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", solver_options={"polish_long": True, "polish_iters": 40})
    rates = opt.solve(sl, infra)
    ref, _, cert = solve_certified(build_reference_problem(sl, infra, iface, spec, "SOC"))
    assert cert is not None and cert.worst < 1e-7
    res = opt.last_result
    print(f"[polish-long] public surface: iters {int(res.iters[0])} (plain handle {int(plain.last_result.iters[0])}), status {int(res.status[0])}, "
          f"|x - x_ipm| {np.abs(rates - ref).max():.2e} A")
    assert int(res.status[0]) == 1 and 40 < int(res.iters[0]) <= 40 + LC.WINDOW, int(res.iters[0])   # handed over at 40, polished
    assert int(plain.last_result.iters[0]) > int(res.iters[0])   # (the same snapshot without the switch: the ADMM runs on; measured 140 against 42)
    assert np.abs(rates - ref).max() <= RATE_TOL, np.abs(rates - ref).max()
    # the handle cache is keyed on the switch: the plain optimizer still has its own handle, and its answer
    before = (int(plain.last_result.iters[0]), plain.last_result.x.copy())
    plain.solve(sl, infra)
    assert int(plain.last_result.iters[0]) == before[0] and np.array_equal(plain.last_result.x, before[1])
