"""The ground truth of tests/verdict_cases.py is true, and the CPU twins agree with it (no GPU needed).

Every probe sits at a relative offset d in +-{1e-2, 1e-3, 1e-4, 1e-5} from the feasibility boundary of its family.
  * every witness satisfies box, energy, site and peak rows in plain fp64 numpy; every Farkas vector proves
    infeasibility; every EMPTY_SET case has a session whose bounds miss its energy row;
  * the analytic threshold is the optimum of the max-theta LP (scipy HiGHS) where the LP exists (LINEAR);
  * oracle/admm_port at the library's default options decides every probe as the truth says, except the probes recorded in
    ``verdict_cases.TWIN_UNDECIDED`` -- at most one in twenty per family, never a feasible one (none at present);
  * family (d), sites.caltech54(): the LP's scaled schedule is a witness in both cones, its dual vector bounds theta in
    LINEAR, and the SOC threshold comes from oracle.ipm (held to the accuracy it reaches, 1e-4);
  * oracle/admm_ref, the numpy restatement, gives the C twin's verdict on the small cases of (a) to (c)."""
import functools

import numpy as np
import pytest

from tests import verdict_cases as V

UNDECIDED_SHARE = 1.0 / 20.0   # per family (the issue's quota)


@functools.lru_cache(maxsize=None)
def _cases(family):
    return V.FAMILIES[family]()


@functools.lru_cache(maxsize=None)
def _twin(family):
    """status and iterations of oracle/admm_port at the library's defaults (accel_mem 5) on every case of a family"""
    from oracle import admm_port

    out = [admm_port.solve_batch(c.batch, threads=1, accel_mem=5) for c in _cases(family)]
    return [(int(o["status"][0]), int(o["iters"][0])) for o in out]


@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_the_grid_is_the_one_stated(family):
    cases = _cases(family)
    assert len({c.name for c in cases}) == len(cases)
    by_d = {}
    for c in cases:
        by_d.setdefault(c.d, []).append(c)
        assert c.truth == ("feasible" if c.d < 0 else ("empty_set" if family == "e" else "infeasible")), c.name
        assert c.batch.B == 1 and (c.batch.presolve_status is None or not c.batch.presolve_status.any()), c.name
    assert sorted(by_d) == sorted(V.PROBES)
    if family == "d":   # SOC has no infeasible probe below d = 1e-3 (the conic oracle's accuracy)
        assert all(c.d < 0 or c.d >= 1e-3 for c in cases if c.cone == "SOC") and {c.cone for c in cases} == {"LINEAR", "SOC"}
    else:
        assert len({len(v) for v in by_d.values()}) == 1


@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_every_witness_is_feasible_and_every_proof_holds(family):
    for c in _cases(family):
        if c.truth == "feasible":
            v = V.violation(c, c.evidence["witness"])
            assert v <= 0.0, (c.name, v)
        elif c.truth == "infeasible" and family == "d" and c.cone == "SOC":
            # no linear proof on a three-phase cone: theta* comes from the interior-point oracle.  It stalls on this
            # degenerate program short of its 1e-9 tolerance; what it reaches is held to 1e-4, a tenth of the nearest probe
            theta, res = V.d_theta_soc(int(c.name.split("_s")[1][0]))
            print(f"[verdict] {c.name}: theta*_SOC {theta:.6f} ({res.status}, gap {res.gap:.1e}, pres {res.pres:.1e}, dres {res.dres:.1e})")
            assert max(abs(res.gap), res.pres, res.dres) <= 1e-4 and res.status != "primal_infeasible", (c.name, res)
            assert theta >= V._d_base(int(c.name.split("_s")[1][0]))["theta_lin"], c.name   # the SOC set contains the LINEAR one
        elif c.truth == "infeasible" and family == "d":
            m = V.farkas_margin(c)   # weak duality: theta <= theta*_LP; the margin is theta*_LP d
            assert m >= 0.5 * c.d * 0.5, (c.name, m)
        elif c.truth == "infeasible":
            m = V.farkas_margin(c)
            # the margin is (demand - limit) summed over the proof's periods: at least |d| x the smallest limit here
            assert m >= 0.5 * abs(c.d) * 30.0, (c.name, m)
        else:
            m = V.empty_margin(c)
            assert m >= 0.5 * abs(c.d) * 6.0, (c.name, m)


def _max_theta_lp(case):
    """max theta s.t. energy rows == theta cap, site rows and peak, box: the largest uniform scaling of the case's demands
    that has a schedule (LINEAR cases with equality rows and lb = 0).  Returns theta*."""
    from scipy.optimize import linprog

    b = case.batch
    N, T = b.N, int(b.T[0])
    assert b.s_eq[0] and not b.lb.any() and case.cone == "LINEAR"
    nv = N * T + 1
    Aeq, A, rhs = [], [], []
    for k in range(b.K):
        for i in range(N):
            n, o = int(b.s_len[0, k, i]), int(b.s_off[0, k, i])
            if n > 0:
                row = np.zeros(nv); row[i * T + o:i * T + o + n] = 1.0; row[-1] = -float(b.s_cap[0, k, i])
                Aeq.append(row)
    G, lim = b.site.G[:b.site.M], b.site.limits
    for t in range(T):
        for j in range(b.site.M):
            row = np.zeros(nv); row[np.arange(N) * T + t] = G[j]
            A.append(row); rhs.append(lim[j])
        if b.peak is not None and np.isfinite(b.peak[0, t]):
            row = np.zeros(nv); row[np.arange(N) * T + t] = 1.0
            A.append(row); rhs.append(b.peak[0, t])
    c = np.zeros(nv); c[-1] = -1.0
    bounds = [(0.0, float(u)) for u in b.ub[0, :, :T].ravel()] + [(0.0, None)]
    res = linprog(c, A_ub=np.array(A), b_ub=np.array(rhs), A_eq=np.array(Aeq), b_eq=np.zeros(len(Aeq)), bounds=bounds, method="highs")
    assert res.status == 0, res.message
    return float(res.x[-1])


@pytest.mark.parametrize("make", [lambda d: V.feeder_equalities("n2", "LINEAR", d), lambda d: V.feeder_equalities("n8", "LINEAR", d),
                                  lambda d: V.feeder_equalities("pods18", "LINEAR", d), lambda d: V.peak_cause("n8", "LINEAR", d, "eq")])
def test_analytic_threshold_is_the_lp_optimum(make):
    """demands limit (1 + d) scaled by theta have a schedule iff theta <= 1 / (1 + d): HiGHS finds that theta*"""
    for d in (-1e-2, 1e-2, 1e-5):
        theta = _max_theta_lp(make(d))
        assert abs(theta * (1 + d) - 1.0) <= 1e-9, (d, theta)


@pytest.mark.parametrize("family", list(V.FAMILIES))
def test_c_twin_decides_every_probe(family):
    cases, twin = _cases(family), _twin(family)
    off = {c.name: st for c, (st, _) in zip(cases, twin) if st != V.STATUS_OF[c.truth]}
    recorded = {c.name: V.TWIN_UNDECIDED[c.name] for c in cases if c.name in V.TWIN_UNDECIDED}
    print(f"[verdict] family {family}: {len(cases)} probes, {len(recorded)} recorded as undecided by the twin")
    assert off == recorded, (off, recorded)
    assert len(recorded) <= UNDECIDED_SHARE * len(cases)
    for c, (st, it) in zip(cases, twin):
        if c.truth == "feasible":
            assert st == 1, (c.name, st)   # a feasible probe ending 3 or 4 in the twin is a bug, never a record
        if st == 3:
            assert it < 5000, (c.name, it)
        if st == 4:
            assert it == 0, (c.name, it)


def test_recorded_probes_exist():
    names = {c.name for f in V.FAMILIES for c in _cases(f)}
    assert set(V.TWIN_UNDECIDED) <= names


@pytest.mark.parametrize("family", ["a", "b", "c", "e"])
def test_numpy_restatement_gives_the_c_twins_verdict(family):
    from oracle.admm_ref import AdmmOptions, solve_one

    picked = [(c, tw) for c, tw in zip(_cases(family), _twin(family)) if c.site in V.SMALL_SITES]
    assert len(picked) >= 16
    for c, (st, it) in picked:
        out = solve_one(c.batch, 0, AdmmOptions(eps_abs=1e-8, eps_rel=1e-8, reg_rel=0.06, accel_mem=5))
        assert int(out["status"]) == st, (c.name, int(out["status"]), st)
        if st == 3:
            assert abs(int(out["iters"]) - it) <= 20, (c.name, int(out["iters"]), it)
