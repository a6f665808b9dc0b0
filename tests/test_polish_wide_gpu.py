"""``polish_wide_kernel`` (adacharge_amd/csrc/acn_qp_polish_wide.hpp: 64 < N <= 1,024, horizons <= 48) held to the polish's
specification oracle/polish_ref.py, problem by problem, on the cases of tests/polish_wide_cases.py (tests/test_polish_wide_cases.py
proves them fit on the CPU).  The wide polish runs BEHIND the solver launch, so every case at every padded shape gets two
launches with poisoned outputs and the multipliers asked for, under the case's start options and retry_passes = 0:
  off     a plain handle                -- the hand-over point: x, y of what ended MAX_ITER (2) or SOLVED_INACCURATE (5)
  on      a ``polish_wide=True`` handle -- the same launch, followed by the list, polish and restore kernels
The specification starts from ``off``'s x, y of each listed problem, with its MAX_ROWS raised to the worst case of the
shape (the kernel's tables hold it: none is given up for `rows`).  WHO WAS POLISHED is what ``on`` ends SOLVED that
``off`` did not; every other problem of ``on`` must carry the bits of ``off``."""
import collections
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import polish_cases as PC
from tests import polish_wide_cases as WC

CASES = list(WC.CASES)
KEYS = ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")
COUNTERS = ("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt")
WHY = {"rows": "gave_up_rows", "pivot": "gave_up_pivot", "rounds": "gave_up_rounds", "verify": "gave_up_kkt"}
X_TOL = 1e-7      # A   (tests/test_polish_gpu.py's constants)
Y_REL = 2e-3
# pri_res / dua_res of a polished problem against the specification's primal / stat, in units of the acceptance limits of the
# final check (1e-8 and 1e-8 max(1, |q|_inf)): 10x the worst measured on an MI355X [in brackets]
RES_TOL = {"pri": 3.6e-4, "dua": 1.6e-3}   # [3.59e-5 (n512_soc_late), 1.56e-4 (n72_soc_multi)]
# problems on which the kernel and the specification may disagree about acceptance, with the reason (at most one per case)
DISAGREE = {}


@functools.lru_cache(maxsize=None)
def _ran(case):
    from adacharge_amd.backend import SiteHandle, default_options

    pool = WC.pool(WC.CASES[case][0])
    off, on = SiteHandle(pool.site, 0), SiteHandle(pool.site, 0, polish_wide=True)
    o = default_options(**WC.start_options(case))
    runs = []
    for t, k in WC.shapes(case):
        fam, pol = on.route(t, k, pool.B)
        assert (fam, pol) == ("stream", 1) and off.route(t, k, pool.B) == ("stream", 0), (case, t, k, fam, pol)
        padded = H.pad_batch(pool, t, k)
        a = H.launch_poisoned(off, padded, o)
        s0 = on.polish_stats()
        b = H.launch_poisoned(on, padded, o)
        s1 = on.polish_stats()
        listed = [int(p) for p in np.flatnonzero(np.isin(a["status"], (2, 5)))]
        runs.append(dict(shape=(t, k), padded=padded, off=a, on=b, listed=listed, stats={c: s1[c] - s0[c] for c in COUNTERS},
                         rounds=s1.get("rounds", 0) - s0.get("rounds", 0)))
    off.close()
    on.close()
    res = iter(WC.spec_many([WC.spec_job(pool, p, r["off"]["x"][p], r["off"]["y"][p], r["shape"][0]) for r in runs for p in r["listed"]]))
    for r in runs:
        r["spec"] = {p: next(res) for p in r["listed"]}
        r["owed"] = {p: ("accept" if info["ok"] else info["why"]) for p, (_, info) in r["spec"].items()}
        r["polished"] = [p for p in range(pool.B) if r["on"]["status"][p] == 1 and r["off"]["status"][p] != 1]
    return pool, runs


def _where(case, r):
    return f"{case} (t_max {r['shape'][0]}, K {r['shape'][1]})"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_the_list_is_what_the_solver_left_open_and_the_counters_add_up(case):
    pool, runs = _ran(case)
    for r in runs:
        print(f"[polish-wide] {_where(case, r)}: listed {len(r['listed'])}, polished {len(r['polished'])}, {r['stats']}")
        for key in ("x", "y", "pri_res", "dua_res", "obj"):
            for run in ("off", "on"):
                assert not np.isnan(r[run][key]).any(), f"{_where(case, r)}: {run} {key} left unwritten"
        assert r["listed"] and set(r["polished"]) <= set(r["listed"]), (_where(case, r), r["listed"], r["polished"])
        assert r["stats"]["attempted"] == len(r["listed"]), (_where(case, r), r["stats"], r["listed"])
        assert r["stats"]["solved"] == len(r["polished"]), (_where(case, r), r["stats"], r["polished"])
        assert sum(r["stats"][c] for c in COUNTERS[1:]) == r["stats"]["attempted"] and r["stats"]["gave_up_rows"] == 0, (_where(case, r), r["stats"])
        assert not np.isin(r["on"]["status"], (0, 6)).any(), (_where(case, r), r["on"]["status"])   # (6: the internal mark)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_the_kernel_polishes_exactly_what_the_specification_accepts(case):
    pool, runs = _ran(case)
    allowed = set(DISAGREE.get(case, {}))
    for r in runs:
        accepted = {p for p, w in r["owed"].items() if w == "accept"}
        odd = accepted ^ set(r["polished"])
        why = collections.Counter(w for w in r["owed"].values() if w != "accept")
        print(f"[polish-wide] {_where(case, r)}: owed: accept {len(accepted)}, give up {dict(why)}; kernel {r['stats']}; disagree {sorted(odd)}")
        assert odd <= allowed and len(odd) <= 1, (_where(case, r), sorted(odd), {p: {k: v for k, v in r["spec"][p][1].items() if k != "y"} for p in odd})
        for reason, counter in WHY.items():
            assert abs(r["stats"][counter] - why.get(reason, 0)) <= len(odd), (_where(case, r), reason, r["stats"], dict(why))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_polished_answers_are_the_specifications(case):
    pool, runs = _ran(case)
    late = WC.CASES[case][3]
    worst = dict(x=0.0, y=0.0, pri=0.0, dua=0.0)
    for r in runs:
        out = r["on"]
        for p in r["polished"]:
            xs, info = r["spec"][p]
            if r["owed"][p] != "accept":
                continue
            T = xs.shape[1]
            x, y = out["x"][p], out["y"][p]
            assert not x[:, T:].any() and not y[:, T:].any(), (_where(case, r), p)
            qn = max(1.0, float(np.abs(pool.q[p]).max()))
            rounds = int(out["iters"][p]) - int(r["off"]["iters"][p])
            d = dict(x=float(np.abs(x[:, :T] - xs).max()),
                     y=float(np.abs(y[:, :T] - info["y"]).max()) / max(1.0, float(np.abs(info["y"]).max())),
                     pri=abs(float(out["pri_res"][p]) - max(info["primal"], 0.0)) / 1e-8,
                     dua=abs(float(out["dua_res"][p]) - info["stat"]) / (1e-8 * qn))
            worst = {k: max(worst[k], v) for k, v in d.items()}
            print(f"[polish-wide] {_where(case, r)} problem {p}: {d}, rounds {rounds} (specification {info['rounds']})")
            assert d["x"] <= X_TOL and d["y"] <= Y_REL, (_where(case, r), p, d)
            assert 0 < rounds <= WC.WINDOW, (_where(case, r), p, rounds)
            if late:
                assert rounds == info["rounds"], (_where(case, r), p, rounds, info["rounds"])
            assert d["pri"] <= RES_TOL["pri"] and d["dua"] <= RES_TOL["dua"], (_where(case, r), p, d)
    print(f"[polish-wide] {case}: worst |x - x_spec| {worst['x']:.2e} A, y {worst['y']:.2e} relative, pri_res {worst['pri']:.2e} and dua_res "
          f"{worst['dua']:.2e} of the check's limits")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_everything_else_keeps_the_bits_of_the_plain_launch(case):
    """the problems the ADMM solved, the ones the polish gave up (the rejected instance of n80_lin_peak, all of n257_soc_rounds)"""
    pool, runs = _ran(case)
    for r in runs:
        rest = [p for p in range(pool.B) if p not in r["polished"]]
        for key in KEYS:
            for p in rest:
                assert np.array_equal(r["on"][key][p], r["off"][key][p]), (_where(case, r), p, key)


@pytest.mark.gpu
def test_cases_reach_both_cones_a_peak_row_four_sessions_three_tiles_and_the_give_ups_of_the_table():
    kinds, gave = set(), collections.Counter()
    for case in CASES:
        pool, runs = _ran(case)
        site = pool.site
        for r in runs:
            gave.update({c: r["stats"][c] for c in COUNTERS[2:]})
            for p in r["polished"]:
                kinds.add("soc" if int(site.cone) == 1 else "linear")
                kinds.add(f"tiles_{min((site.N + 63) // 64, 3)}")
                if site.has_peak:
                    kinds.add("peak_row")
                if pool.K == 4 and pool.s_len[p, 3].any():
                    kinds.add("four_sessions")
                if site.N == 1024 and np.abs(r["on"]["x"][p][960:]).max() > 0:
                    kinds.add("last_tile")
    print(f"[polish-wide] {sorted(kinds)}, give-ups {dict(gave)}")
    assert {"soc", "linear", "peak_row", "four_sessions", "tiles_2", "tiles_3", "last_tile"} <= kinds, sorted(kinds)
    assert gave["gave_up_rounds"] and gave["gave_up_kkt"] and not gave["gave_up_rows"], dict(gave)


@pytest.mark.gpu
def test_same_bits_alone_and_at_any_position_of_a_batch_five_times_the_size():
    """twenty listed problems on sixteen slabs: the queue hands a workgroup a second problem"""
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import ProblemBatch

    case = "n65_soc"
    pool = WC.pool(WC.CASES[case][0])
    h = SiteHandle(pool.site, 0, polish_wide=True)
    o = default_options(**WC.start_options(case))
    alone = H.launch_poisoned(h, pool, o)
    s0 = h.polish_stats()
    five = H.launch_poisoned(h, ProblemBatch.concatenate([pool] * 5), o)
    s1 = h.polish_stats()
    h.close()
    assert s1["attempted"] - s0["attempted"] == 5 * 4 and s1["solved"] - s0["solved"] == 5 * 4, (s0, s1)
    for key in KEYS:
        for part in range(5):
            assert np.array_equal(five[key][part * pool.B:(part + 1) * pool.B], alone[key]), (key, part)


@pytest.mark.gpu
def test_the_switch_costs_no_bit_where_nothing_is_listed_or_polish_iters_is_zero():
    from adacharge_amd.backend import SiteHandle, default_options

    case = "n65_soc"
    pool = WC.pool(WC.CASES[case][0])
    off, on = SiteHandle(pool.site, 0), SiteHandle(pool.site, 0, polish_wide=True)
    s0 = on.polish_stats()
    a, b = H.launch_poisoned(off, pool, default_options()), H.launch_poisoned(on, pool, default_options())
    assert (a["status"] == 1).all(), a["status"]   # default options: every problem SOLVED, nothing listed
    assert on.polish_stats()["attempted"] == s0["attempted"]
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    o = default_options(polish_iters=0, **WC.start_options(case))   # problems left open, and no polish anywhere
    a, b = H.launch_poisoned(off, pool, o), H.launch_poisoned(on, pool, o)
    assert np.isin(a["status"], (2, 5)).any() and on.polish_stats()["attempted"] == s0["attempted"]
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    off.close()
    on.close()


@pytest.mark.gpu
def test_through_the_public_surface_the_key_returns_the_polished_schedule_and_its_absence_the_plain_one():
    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, quick_charge, sites, total_energy
    from adacharge_amd.acn import Interface

    case = "n65_soc"
    pool, runs = _ran(case)
    r = runs[0]
    infra = PC._infra((65, 4, 0.5))   # the pool's snapshots again (tests/polish_cases.py: site_pool)
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(81)
    snaps = [sites.random_sessions_general(infra, (8, 6, 7)[k % 3], rng, two_per_evse=False, min_rates=True, demand_scale=1.5) for k in range(6)]
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3), ObjectiveComponent(total_energy, 0.5)]
    start = WC.start_options(case)
    plain = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", solver_options=dict(start))
    _, st_plain = plain.solve_batch(snaps, infra)
    opt = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", solver_options=dict(start, polish_wide=True))
    rates, st = opt.solve_batch(snaps, infra)
    print(f"[polish-wide] public surface: status {list(map(int, st))} (plain {list(map(int, st_plain))}), iters {opt.last_result.iters.tolist()}")
    assert np.array_equal(st_plain, r["off"]["status"]) and np.array_equal(st, r["on"]["status"]), (st_plain, st)
    assert np.array_equal(plain.last_result.iters, r["off"]["iters"]) and np.array_equal(opt.last_result.iters, r["on"]["iters"])
    for p in range(pool.B):
        T = int(pool.T[p])
        assert np.abs(np.asarray(rates[p])[:, :T] - r["on"]["x"][p][:, :T]).max() <= X_TOL, p
        assert np.abs(plain.last_result.x[p][:, :T] - r["off"]["x"][p][:, :T]).max() <= X_TOL, p
    # the handle cache is keyed on the switch: the plain optimizer still has its own handle, and its answer
    before = plain.last_result.x.copy()
    plain.solve_batch(snaps, infra)
    assert np.array_equal(plain.last_result.x, before) and np.array_equal(plain.last_result.status, st_plain)
