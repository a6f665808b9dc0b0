"""The pools of tests/polish_cases.py are fit for the job before a GPU sees them (CPU; the twin oracle/admm_port hands over,
oracle/polish_ref.py polishes): every case hands at least eight problems over, the specification accepts three quarters of
the feasible ones (or gives up for the reason the case is there for), what it accepts is an optimum -- the KKT certificate
at the SOLVED constants, and the twin's answer (TWIN_EPS below) to 1e-7 A -- padding in t_max and K changes none of its
bits, and the set whose verdict or round count moves with the start point (ROUND_FRAGILE) stays below half of every late
case.  tests/test_polish_gpu.py holds the kernel to the same specification from the device's own hand-over points."""
import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests import polish_cases as PC

CASES = list(PC.CASES)
# The twin the accepted answers are held to, to 1e-7 A.  At eps_abs = eps_rel = 1e-10 the twin itself is up to 2.6e-7 A from
# the optimum on nine of these problems (ct54_lin_eq_peak 13: 2.2e-7, jpl_soc_t17 0: 2.3e-7 and 2: 2.6e-7, ct54_soc_peak_one
# 8: 2.0e-7, ...): tightened to 1e-12 it moves TOWARDS the specification's answer (5.4e-9, 2.5e-8, 1.6e-9 A on the first
# three), with and without Anderson columns.  So the reference is the twin at 1e-12 and the bound stays at 1e-7 A.
TWIN_EPS = 1e-12


def _padded_answer(batch, b, x, y):
    T = x.shape[1]
    xp, yp = np.zeros((batch.N, batch.Tm)), np.zeros((batch.site.Mg, batch.Tm))
    xp[:, :T], yp[:, :T] = x, y
    return xp, yp


@pytest.mark.parametrize("case", CASES)
def test_case_hands_enough_over_and_the_specification_does_what_the_case_is_for(case):
    name, P, expect, late = PC.CASES[case]
    assert P % PC.CHECK_EVERY == 0
    batch, c = PC.pool(name), PC.cpu_case(case)
    assert 8 <= batch.B <= 32
    index, spec, final = c["index"], c["spec"], c["final"]["status"]
    feasible = [b for b in spec if final[b] != 3]
    ok = [b for b in feasible if spec[b][1]["ok"]]
    why = {b: spec[b][1]["why"] for b in spec}
    rounds = [spec[b][1]["rounds"] for b in ok]
    print(f"[polish-cases] {case}: not SOLVED at P {len(index)}, declined {c['declined']}, accepted {len(ok)} of {len(feasible)} feasible, "
          f"why {sorted(why.items())}, rounds of the accepted {sorted(rounds)}, fragile {c['fragile']}")
    assert len(index) >= 8, index
    if expect == "rows":
        assert len(c["declined"]) >= 4, c["declined"]
    elif expect == "rounds":
        assert sum(w == "rounds" for w in why.values()) >= 3 and len(ok) >= 3, why
    elif expect == "verify":
        assert sum(why[b] == "verify" for b in feasible) >= 5 and len(ok) >= 5, why
    else:
        assert len(ok) >= 0.75 * len(feasible), (len(ok), len(feasible), why)
    # the infeasible problems that are still uncertified at P: the specification gives up on every one
    for b in spec:
        if final[b] == 3:
            assert not spec[b][1]["ok"], (case, b, spec[b][1])
    assert c["fragile"] == PC.ROUND_FRAGILE.get(case, ()), (case, c["fragile"])
    if late:
        assert 2 * len(c["fragile"]) < len(index), (c["fragile"], index)
    elif expect == "accept":
        assert max(rounds) >= 10, rounds   # an early hand-over: a poor first working set


def test_infeasible_problems_reach_the_polish_uncertified():
    """two cases carry problems the twin ends PRIMAL_INFEASIBLE and that are not certified at P"""
    n = 0
    for case in ("ct54_lin_eq_peak@20", "n64_lin_t16_peak@100"):
        c = PC.cpu_case(case)
        n += sum(c["final"]["status"][b] == 3 for b in c["spec"])
    assert n >= 3, n


@pytest.mark.parametrize("case", CASES)
def test_what_the_specification_accepts_is_the_optimum(case):
    name, P, _, _ = PC.CASES[case]
    batch, c = PC.pool(name), PC.cpu_case(case)
    tight = PC.twin(name, eps=TWIN_EPS)
    worst = 0.0
    for b, (x, info) in c["spec"].items():
        if not info["ok"]:
            continue
        T = x.shape[1]
        xp, yp = _padded_answer(batch, b, x, info["y"])
        obj = float(((0.5 * batch.pdiag[b] * xp + batch.q[b]) * xp).sum())
        bad = kkt.failures(kkt.certify(batch, b, xp, yp, obj), 1)
        assert not bad, (case, b, bad)
        assert tight["status"][b] == 1, (case, b, int(tight["status"][b]))   # every accepted answer is compared
        d = float(np.abs(x - tight["x"][b][:, :T]).max())
        worst = max(worst, d)
        assert d <= 1e-7, (case, b, d)
    print(f"[polish-cases] {case}: worst |x_spec - x_twin({TWIN_EPS:g})| {worst:.2e} A")


@pytest.mark.parametrize("case", CASES)
def test_padding_changes_none_of_the_specifications_bits(case):
    """the specification reads batch.T[b]: a sample, the two cheapest problems of every case padded to t_max = 32 and K = 4.
    (The GPU file does not lean on it: it hands the specification the unpadded pool with x and y cut to the horizon, and runs
    it once per DISTINCT device hand-over point, whatever the padding that produced it.)"""
    name, P, _, _ = PC.CASES[case]
    batch, c, at = PC.pool(name), PC.cpu_case(case), PC.twin(name, P)
    wide = H.pad_batch(batch, 32, 4)
    for b in sorted(c["spec"], key=lambda b: c["spec"][b][1]["rounds"])[:2]:
        x, info = c["spec"][b]
        (xw, iw), = PC.spec_many([PC.spec_args(wide, b, H.pad_result(at["x"][b], 32), H.pad_result(at["y"][b], 32))])
        assert np.array_equal(x, xw) and (info["ok"], info["why"], info["rounds"]) == (iw["ok"], iw["why"], iw["rounds"]), (case, b)
        if info["ok"]:
            assert np.array_equal(info["y"], iw["y"]), (case, b)


def test_cases_cover_what_the_polish_serves():
    """among the problems the specification ACCEPTS: both cones, no / scalar / vector peak, equalities, K = 1, 2, 4 with real
    sessions in slots 1 ... 3, lb > 0, stepped ub, lb == ub inside a window, N = 3, 8, 54, 52, 64, horizons that reach
    both instantiations"""
    seen = set()
    for case in CASES:
        name, P, _, _ = PC.CASES[case]
        batch, c = PC.pool(name), PC.cpu_case(case)
        site = batch.site
        for b, (x, info) in c["spec"].items():
            if not info["ok"]:
                continue
            T = int(batch.T[b])
            seen.add("soc" if int(site.cone) == 1 else "linear")
            if batch.peak is None or not np.isfinite(batch.peak[b][:T]).any():
                seen.add("no_peak")
            else:
                pk = batch.peak[b][:T]
                seen.add("scalar_peak" if np.ptp(pk) == 0 else "vector_peak")
                if np.abs(info["y"][site.Mg - 1]).max() > 0:
                    seen.add("peak_tight")
            seen.add("eq" if batch.s_eq[b] else "ineq")
            seen.add(f"K{batch.K}")
            for k in range(1, batch.K):
                if batch.s_len[b, k].any():
                    seen.add(f"slot{k}")
            win = np.zeros((batch.N, T), bool)
            for k in range(batch.K):
                for i in np.flatnonzero(batch.s_len[b, k]):
                    win[i, batch.s_off[b, k, i]: batch.s_off[b, k, i] + batch.s_len[b, k, i]] = True
            lb, ub = batch.lb[b][:, :T], batch.ub[b][:, :T]
            if (lb[win] > 0).any():
                seen.add("lb_positive")
            if ((lb == ub) & win).any():
                seen.add("pinned")
            if len(np.unique(ub[win])) > 1:
                seen.add("stepped_ub")
            seen.add(f"N{batch.N}")
            seen.add("tq8" if batch.Tm > 16 else "tq4")
    want = {"soc", "linear", "no_peak", "scalar_peak", "vector_peak", "peak_tight", "eq", "ineq", "K1", "K2", "K4", "slot1", "slot2",
            "slot3", "lb_positive", "pinned", "stepped_ub", "N3", "N8", "N54", "N52", "N64", "tq4", "tq8"}
    assert want <= seen, sorted(want - seen)


def test_restated_lds_tables_of_the_polish_kernel():
    """polish_cases.polish_tables (PolishLds and polish_plan's LDS budget, restated; tests/test_polish_plan.py holds it to
    the headers, tests/test_polish_gpu.py to acnqp_route on every shape it runs): no block fits for SOC rows at N = 64 and t_max = 32, so the library runs no polish
    there and polish_kernel<8> over 32 periods is held on N = 52; the LINEAR N = 64 site fits at 32; four session slots leave
    jpl52 at t_max = 32 less room for blocks than two -- and problems of the rows case outgrow it"""
    soc64 = PC.site_pool((64, 4, 0.4), "SOC", (32,), 1, 1).site
    assert PC.polish_tables(soc64, 32, 2, False)[2] == -1 and PC.polish_tables(soc64, 32, 4, False)[2] == -1
    assert PC.polish_tables(soc64, 29, 2, False)[2] > 0
    assert PC.polish_tables(PC.pool("n64_lin_t16_peak").site, 32, 4, True)[2] > 0
    jpl = PC.pool("jpl_soc_t32_rows").site
    two, four = PC.polish_tables(jpl, 32, 2, False), PC.polish_tables(jpl, 32, 4, False)
    assert (two[0], two[1], four[0], four[1]) == (256, 104, 256, 128) and 0 < four[2] < two[2], (two, four)
    spec = PC.cpu_case("jpl_soc_t32_rows@40")["spec"]
    grown = [b for b, (_, info) in spec.items() if PC.outgrows(info, four) and not PC.outgrows(info, two)]
    print(f"[polish-cases] jpl52 at t_max 32: tables K = 2 {two}, K = 4 {four}; outgrow K = 4 only: {grown}, "
          f"blocks {[spec[b][1]['blocks'] for b in spec]}, sessions {[spec[b][1]['sessions'] for b in spec]}")
    assert grown, {b: (info["blocks"], info["sessions"]) for b, (_, info) in spec.items()}
