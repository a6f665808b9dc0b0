"""The dual report's SPECIFICATION (tests/duals_spec.py) on the CPU, and the additive C ABI of the report.

  * on the C twin's answers for the six pools of tests/test_kkt_certificate.py the specification's multipliers satisfy the
    explicit KKT conditions elementwise, and its ``stat`` is oracle/kkt.py's (exact water-filling against a 200-step
    bisection: two computations of one quantity);
  * the multiplier means what it claims: ``mu / k_i`` equals the dual the interior-point oracle gives the session's energy
    row, on eight strictly convex cases of tests/golden/caltech54_T12.npz;
  * three corruptions of a passing answer move the residual they should;
  * the ABI version is still 10, a null handle is refused (the layout of ``acnqp_duals``: tests/test_abi.py).
tests/test_duals_gpu.py holds the kernel to this specification."""
import ctypes as C

import numpy as np
import pytest

from oracle import kkt
from tests import duals_spec as DS
from tests import helpers as H
from tests.test_kkt_certificate import POOLS, _solved

ROUNDOFF = 1e-12   # x max(1, |q|_inf): identities of the definition


def _windows(batch, b):
    for k in range(batch.K):
        for i in range(batch.N):
            L, o = int(batch.s_len[b, k, i]), int(batch.s_off[b, k, i])
            if L > 0:
                yield k, i, slice(o, o + L)


@pytest.mark.parametrize("name", list(POOLS))
def test_specification_satisfies_the_kkt_conditions_elementwise(name):
    batch, out = _solved(name)
    for b in range(batch.B):
        x, y = out["x"][b], out["y"][b]
        d = DS.duals(batch, b, x, y)
        mu, z, g = d["mu"], d["z"], d["g"]
        stat, qs = d["res"][0], max(1.0, d["qn"])
        lb = batch.lb[b]
        ub = np.maximum(batch.ub[b], lb)
        inside = np.zeros(x.shape, bool)
        for k, i, w in _windows(batch, b):
            inside[i, w] = True
            # g + mu + z = 0: an identity of the definition
            assert np.abs(g[i, w] + mu[k, i] + z[i, w]).max() <= ROUNDOFF * qs, (name, b, k, i)
            if not batch.s_eq[b]:
                assert mu[k, i] >= 0.0, (name, b, k, i, mu[k, i])
                # |sum clip(v - mu) - sum x| <= L stat: a row with more slack than that has mu = 0
                slack = float(batch.s_cap[b, k, i]) - float(x[i, w].sum())
                if slack > (w.stop - w.start) * stat + ROUNDOFF * max(1.0, abs(float(batch.s_cap[b, k, i]))):
                    assert mu[k, i] == 0.0, (name, b, k, i, slack, mu[k, i])
        assert not z[~inside].any() and not z[:, int(batch.T[b]):].any()
        # z > 0 only where x = ub, z < 0 only where x = lb, up to the natural residual (x = clip(x + z) up to stat)
        assert (np.minimum(np.maximum(z, 0.0), ub - x) <= stat + ROUNDOFF * 64).all(), (name, b)
        assert (np.minimum(np.maximum(-z, 0.0), x - lb) <= stat + ROUNDOFF * 64).all(), (name, b)
        # stat: the exact water-filling against the oracle's bisection.  Both are |x - p| with x, p up to 80 A whose last
        # bits differ (the bisection ends within an ulp of its shift): 1e-12 A
        c = kkt.certify(batch, b, x, y, out["obj"][b])
        assert abs(stat - c["stat"] * qs) <= 1e-12, (name, b, stat, c["stat"] * qs)
        assert d["res"][1] == pytest.approx(c["energy"], abs=1e-15)
        assert d["res"][2] == pytest.approx(c["site"], abs=1e-15)
        assert d["res"][3] == pytest.approx(c["comp"], abs=1e-15)


def test_unsolved_problem_gets_zeros_and_infinite_residuals():
    batch, out = _solved("ct54_lin_t12_vpeak")
    d = DS.duals(batch, 0, out["x"][0], out["y"][0], status=kkt.ST_MAX_ITER)
    assert not d["mu"].any() and not d["z"].any() and np.isposinf(d["res"]).all()


def test_waterfill_tie_rule_and_unreachable_caps():
    lb, ub = np.array([0.0, 8.0, 0.0]), np.array([32.0, 32.0, 16.0])
    # every entry on ub, cap = sum ub: admissible (-inf, min(v - ub)]: the value of least magnitude
    assert DS.waterfill(np.array([40.0, 50.0, 20.0]), lb, ub, 80.0, True) == 0.0
    assert DS.waterfill(np.array([30.0, 50.0, 20.0]), lb, ub, 80.0, True) == -2.0
    assert DS.waterfill(np.array([40.0, 50.0, 20.0]), lb, ub, 80.0, False) == 0.0
    # every entry on lb
    assert DS.waterfill(np.array([-1.0, 3.0, -5.0]), lb, ub, 8.0, True) == 0.0
    assert DS.waterfill(np.array([4.0, 3.0, -5.0]), lb, ub, 8.0, True) == 4.0
    # interior flat segment: entries 0 on ub and 2 on lb for mu in [5, 8], entry 1 fixed
    fl, fu = np.array([0.0, 8.0, 0.0]), np.array([32.0, 8.0, 16.0])
    assert DS.waterfill(np.array([40.0, 0.0, 5.0]), fl, fu, 40.0, True) == 5.0
    assert DS.waterfill(np.array([40.0, 0.0, -3.0]), fl, fu, 40.0, True) == 0.0
    # a plain interior root: two free entries
    assert DS.waterfill(np.array([10.0, 8.0, 12.0]), np.zeros(3), np.full(3, 32.0), 24.0, True) == pytest.approx(2.0)
    assert DS.waterfill(np.array([10.0, 8.0, 12.0]), np.zeros(3), np.full(3, 32.0), 36.0, False) == 0.0


# ---- the multiplier is the energy row's dual -----------------------------------------------------------------------
# Cases: the first eight of caltech54_T12.npz, in fixture order, in which at most half of the sessions have no rate more
# than 1e-3 A inside its bounds (c04 has 19 of 31 such sessions and is left out; shares of the eight: 14/48, 1/48, 20/48,
# 8/48, 7/31, 12/31, 3/31, 4/47).  All are strictly convex (equal_share 1e-3 or 1e-2), LINEAR and SOC.
IPM_CASES = ("c00", "c01", "c02", "c03", "c05", "c06", "c07", "c09")
# |mu / k_i - IPM dual| in $/kWh-equivalent units of the reference's row: 10x the worst difference measured over the eight
# cases (4.83e-3, case c07, on duals of size 35; the others 4e-7 ... 2e-4).  What limits it is the interior-point
# oracle's dual accuracy, not the water-filling: the same answer has stat = 4e-5 A under the IPM's site-row duals.
IPM_DUAL_TOL = 4.9e-2


def ipm_energy_duals(sl, infra, iface, meta, peak=None):
    """(batch, x (N, Tm), y (Mg, Tm), nu (S,)): the case re-solved by oracle/ipm.py -- certified rates, the IPM's site-row
    duals in the row order of the library's G, and its duals of the energy rows (inequality rows: the last block of A_ub)"""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge
    from adacharge_amd.builder import build_batch
    from oracle.ipm import solve_certified
    from oracle.ref_problem import build_reference_problem

    assert not meta["eq"]
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, meta["es"])]
    spec = [("quick_charge", 1, {}), ("equal_share", meta["es"], {})]
    batch = build_batch([sl], infra, iface, obj, meta["ct"], False, peak_limits=[peak])
    prob = build_reference_problem(sl, infra, iface, spec, meta["ct"], False, peak_limit=peak)
    r, res, cert = solve_certified(prob)   # (solve_conic_qp, then the polish)
    assert cert is not None and cert.worst < 1e-7
    zd = res.duals[0]
    N, T, M, l = prob.N, prob.T, batch.site.M, prob.A_ub.shape[0]
    n = N * T
    if meta["ct"] == "SOC":   # cone block (j, t): s = (limit, F x) in Q, dual (z0, z1, z2): the gradient carries -F'(z1, z2)
        zc = zd[l:].reshape(M, T, 3)
        y = np.concatenate([-zc[:, :, 1], -zc[:, :, 2]])
    else:
        y = zd[2 * n:2 * n + M * T].reshape(M, T)
    if peak is not None:
        y = np.concatenate([y, zd[2 * n + (0 if meta["ct"] == "SOC" else M * T):][:T][None, :]])
    nu = zd[l - len(sl):l]
    x = np.zeros((N, batch.Tm))
    x[:, :T] = r
    yy = np.zeros((batch.site.Mg, batch.Tm))
    yy[:, :T] = y
    return batch, x, yy, nu


def unique_sessions(batch, x, sl, infra):
    """[(session index, slot, evse)] of the sessions with at least one rate more than 1e-3 A inside its bounds"""
    out = []
    for k, s in enumerate(sl):
        i = infra.get_station_index(s.station_id)
        w = slice(s.arrival_offset, s.arrival_offset + s.remaining_time)
        ub = np.maximum(batch.ub[0, i, w], batch.lb[0, i, w])
        if ((x[i, w] > batch.lb[0, i, w] + 1e-3) & (x[i, w] < ub - 1e-3)).any():
            slot = int(np.flatnonzero((batch.s_len[0, :, i] > 0) & (batch.s_off[0, :, i] == s.arrival_offset))[0])
            out.append((k, slot, i))
    return out


@pytest.mark.parametrize("key", IPM_CASES)
def test_mu_is_the_dual_of_the_energy_row(key):
    g = H.load_golden()
    infra, iface = H.caltech_interface()
    sl, meta, _ = H.golden_case(g, key)
    assert meta["es"] > 0
    batch, x, y, nu = ipm_energy_duals(sl, infra, iface, meta)
    d = DS.duals(batch, 0, x, y)
    uniq = unique_sessions(batch, x, sl, infra)
    assert len(sl) - len(uniq) <= len(sl) / 2, (key, len(sl), len(uniq))
    worst = 0.0
    for k, slot, i in uniq:
        k_i = infra.voltages[i] * iface.period / 1e3 / 60
        worst = max(worst, abs(d["mu"][slot, i] / k_i - nu[k]))
    print(f"[duals] {key}: {len(uniq)} of {len(sl)} sessions, worst |mu / k - nu| {worst:.3e}, largest dual {np.abs(nu).max():.3g}")
    assert np.abs(nu).max() > 1.0   # (the comparison is not between zeros)
    assert worst <= IPM_DUAL_TOL, (key, worst)


# ---- corruptions move the residual they should ---------------------------------------------------------------------
def _res(batch, b, x, y):
    r = DS.duals(batch, b, x, y)
    return dict(zip(DS.RES_NAMES, r["res"] / np.array([max(1.0, r["qn"]), 1.0, 1.0, 1.0])))


def test_rate_moved_between_free_periods_raises_stat():
    d = 3.2e-3
    batch, out = _solved("ct54_soc_t12_eq_mixedpeak")
    for b in range(batch.B):
        x = out["x"][b]
        for k, i, w in _windows(batch, b):
            free = np.flatnonzero((x[i, w] > batch.lb[b, i, w] + d) & (x[i, w] < batch.ub[b, i, w] - d)) + w.start
            if len(free) >= 2:
                xm = x.copy()
                xm[i, free[0]] += d
                xm[i, free[1]] -= d
                ok, bad = _res(batch, b, x, out["y"][b]), _res(batch, b, xm, out["y"][b])
                assert ok["stat"] <= kkt.STAT_TOL < bad["stat"], (ok, bad)
                assert bad["energy"] <= kkt.EXACT_REL
                return
    pytest.fail("no session with two free periods in the pool")


def test_site_multiplier_scaled_by_1_001_raises_stat():
    for name in ("ct54_lin_t12_vpeak", "ct54_soc_t16_speak"):
        batch, out = _solved(name)
        b = int(np.argmax([np.abs(out["y"][k]).max() for k in range(batch.B)]))
        y = out["y"][b].copy()
        j, t = np.unravel_index(np.argmax(np.abs(y)), y.shape)
        y[j, t] *= 1.001
        ok, bad = _res(batch, b, out["x"][b], out["y"][b]), _res(batch, b, out["x"][b], y)
        assert ok["stat"] <= kkt.STAT_TOL < bad["stat"], (name, ok, bad)


def test_multiplier_on_a_slack_row_raises_comp():
    batch, out = _solved("ct54_lin_t12_vpeak")
    M = batch.site.M
    for b in range(batch.B):
        x, y = out["x"][b], out["y"][b]
        T = int(batch.T[b])
        slack = batch.site.limits[:, None] - batch.site.G[:M] @ x[:, :T]
        j, t = np.unravel_index(np.argmax(slack), slack.shape)
        if slack[j, t] > 1.0 and y[j, t] == 0:
            ym = y.copy()
            ym[j, t] = 1e-4 * np.abs(y).max()
            ok, bad = _res(batch, b, x, y), _res(batch, b, x, ym)
            assert ok["comp"] <= kkt.COMP_TOL < bad["comp"], (ok, bad)
            return
    pytest.fail("no slack row")


# ---- ABI: additive ---------------------------------------------------------------------------------------------------
def test_null_handle_is_refused(hip_library):
    from adacharge_amd import backend

    assert hip_library.acnqp_abi_version() == 10
    d = backend._Duals(None, None, None)
    assert hip_library.acnqp_duals_host(None, None, None, None, None, None, C.byref(d)) == -1
    assert b"acnqp_duals_host" in hip_library.acnqp_last_error() and b"null" in hip_library.acnqp_last_error()
    assert hip_library.acnqp_duals_device(None, None, None, None, None, None, None, None) == -1
    assert b"acnqp_duals_device" in hip_library.acnqp_last_error()
