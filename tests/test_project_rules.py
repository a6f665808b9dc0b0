"""The projection rules of adacharge_amd/csrc/acn_qp_project.hpp (Part 1: what the stream, long and general kernels ask
about their sums), compiled for the host the way tests/test_check_rules.py compiles the check rules.  The shim below
builds a scalar water-filling of one window from NOTHING but those rules -- the sums are plain loops, every decision is
a rule -- and this file holds it against the twin, oracle/admm_ref.py::project_window, which finds the root exactly from
the breakpoints.  Tolerance: the device's own, |sum z - cap| <= proj_tol max(1, |cap|) (the sum taken in the order the
loop takes it, as the device tests its own sum), and every z within that of the twin's.  Two mutations, applied by a -D
of the shim and never by the header, must each fail: the Newton step without its bisection fallback, and the
pinned-at-ub mode taken for inequalities."""
import ctypes
import functools
import math
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

from oracle import admm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")
PROJ_TOL = 1e-13   # Mfma<double>::proj_tol (acn_qp_common.hpp)
BIG = 1e300

SHIM = r"""
#define __host__
#define __device__
#include "acn_qp_project.hpp"
using namespace acnqp;
extern "C" {
int bounds_miss(double sl, double su, double cap, int eq, double proj_tol) { return bounds_miss_energy_row<double>(sl, su, cap, eq != 0, proj_tol); }
// one window, one thread: z = Proj of v onto {lb <= z <= ub, sum z <= (==) cap}; mu0 = the warm multiplier.
// info: [0] mode, [1] steps taken, [2] steps that met a flat piece (nf = 0), [3] the raw bracket started below zero,
// [4] the warm multiplier lay outside the bracket; *m_out: the multiplier (root-find mode only)
void waterfill(int n, const double* v, const double* lb, const double* ub, double cap, int eq_, double mu0, double proj_tol,
               double* z, double* m_out, int* info) {
  const bool eq = eq_ != 0;
  double s0 = 0, sl = 0, su = 0, lo = 1e300, hi = -1e300;
  for (int t = 0; t < n; ++t) {
    z[t] = fmin(fmax(v[t], lb[t]), ub[t]);
    s0 += z[t]; sl += lb[t]; su += ub[t];
    lo = fmin(lo, v[t] - ub[t]); hi = fmax(hi, v[t] - lb[t]);
  }
  const double tol = fill_tol<double>(cap, proj_tol);
#ifdef MUT_UB_FOR_INEQ
  const int mode = fill_mode<double>(n > 0, true, s0, sl, su, cap, tol);
#else
  const int mode = fill_mode<double>(n > 0, eq, s0, sl, su, cap, tol);
#endif
  info[0] = mode; info[1] = info[2] = 0; info[3] = lo < 0; *m_out = 0;
  if (mode == kFillNone) return;
  if (mode == kFillAtUb) { for (int t = 0; t < n; ++t) z[t] = ub[t]; return; }
  if (mode == kFillAtLb) { for (int t = 0; t < n; ++t) z[t] = lb[t]; return; }
  double m = fill_start<double>(eq, mu0, lo, hi);
  info[4] = m != mu0;
  for (int guard = 0; guard <= 100; ++guard) {
    double g = 0, nf = 0;
    for (int t = 0; t < n; ++t) {
      const double u = v[t] - m;
      g += fmin(fmax(u, lb[t]), ub[t]);
      nf += (u > lb[t] && u < ub[t]) ? 1.0 : 0.0;
    }
    const double d = g - cap;
    if (fill_done<double>(d, tol)) break;
    ++info[1];
    if (nf == 0) ++info[2];
#ifdef MUT_NO_BISECT
    double lo_ = -1e300, hi_ = 1e300;   // a bracket that never binds: the plain Newton step
    fill_step<double>(m, d, nf, lo_, hi_, true);
#else
    fill_step<double>(m, d, nf, lo, hi, true);
#endif
  }
  *m_out = m;
  for (int t = 0; t < n; ++t) z[t] = fmin(fmax(v[t] - m, lb[t]), ub[t]);
}
double site_z(int ty, double zh, double lim, double peak, double quad, double soc_scale) { return site_row_z<double>(ty, zh, lim, peak, quad, soc_scale); }
// tau of the demand-charge prox over n periods; returns the steps taken
int dc_tau(int n, const double* zv, double cw, double proj_tol, int guard_max, double* tau_out) {
  double vmax = -1e300;
  for (int t = 0; t < n; ++t) vmax = fmax(vmax, zv[t]);
  double tau = vmax - cw;
  int guard = 0;
  for (;;) {
    ++guard;
    double S = 0, nn = 0;
    for (int t = 0; t < n; ++t) if (zv[t] - tau > 0.0) { S += zv[t] - tau; nn += 1.0; }
    const DcStep<double> s = dc_tau_step<double>(tau, S, nn, cw, vmax, proj_tol, guard, guard_max);
    if (s.fin) break;
    tau = s.tn;
  }
  *tau_out = tau;
  return guard;
}
}
"""

D, I = ctypes.c_double, ctypes.c_int
FREE, BOX, SOC_RE, SOC_IM, PEAK, QUAD, MAX = 0, 1, 2, 3, 4, 5, 6   # row types (acn_qp_check.hpp)
ROOT_FIND, AT_UB, AT_LB, NOTHING = 0, 2, 3, 4                      # kFillRoot, kFillAtUb, kFillAtLb, kFillNone


@functools.lru_cache(maxsize=None)
def _lib(mutation=""):
    tmp = tempfile.mkdtemp(prefix="acnqp_project_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim" + (mutation or "plain") + ".so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, *(["-D" + mutation] if mutation else []), src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    P, PI = ctypes.POINTER(D), ctypes.POINTER(I)
    for name, res, args in (("bounds_miss", I, [D, D, D, I, D]), ("waterfill", None, [I, P, P, P, D, I, D, D, P, P, PI]),
                            ("site_z", D, [I, D, D, D, D, D]), ("dc_tau", I, [I, P, D, D, I, P])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(D))


def _fill(lib, v, lb, ub, cap, eq, mu0=0.0):
    v, lb, ub = (np.ascontiguousarray(a, dtype=np.float64) for a in (v, lb, ub))
    z, m, info = np.empty_like(v), D(0.0), (I * 5)()
    lib.waterfill(len(v), _ptr(v), _ptr(lb), _ptr(ub), cap, int(eq), mu0, PROJ_TOL, _ptr(z), ctypes.byref(m), info)
    return z, SimpleNamespace(mode=info[0], steps=info[1], flat=info[2], lo_below_zero=bool(info[3]), clamped=bool(info[4]), m=m.value)


def _mismatch(lib, v, lb, ub, cap, eq, mu0=0.0):
    """None if the rule-built water-filling meets the device's tolerance and the twin; else what it missed"""
    z, info = _fill(lib, v, lb, ub, cap, eq, mu0)
    zt = admm_ref.project_window(np.asarray(v, float), np.asarray(lb, float), np.asarray(ub, float), cap, eq)
    tol = PROJ_TOL * max(1.0, abs(cap))
    if np.any(z < lb) or np.any(z > ub):
        return "box", z, info
    if info.mode == ROOT_FIND:
        s = 0.0
        for zt_ in z:   # the loop's own order
            s += zt_
        if not abs(s - cap) <= tol:
            return "sum %r against cap %r" % (s, cap), z, info
        if not eq and info.m < 0:
            return "negative multiplier of an inequality", z, info
    if not np.max(np.abs(z - zt), initial=0.0) <= tol:
        return "twin: %r" % float(np.max(np.abs(z - zt))), z, info
    return None


def _random_window(rng, n):
    lb = np.where(rng.random(n) < 0.3, rng.uniform(0.0, 4.0, n), 0.0)
    ub = lb + np.where(rng.random(n) < 0.25, 0.0, rng.uniform(0.0, 32.0, n))
    v = rng.uniform(-8.0, 40.0, n)
    return v, lb, ub


def _sweep_failures(lib):
    """windows of length 1 ... 48, equality and inequality, capacities across and beyond [sum lb, sum ub], warm
    multipliers inside and outside the bracket"""
    rng = np.random.default_rng(20240611)
    bad, modes = [], set()
    for n in range(1, 49):
        for eq in (False, True):
            for rep in range(6):
                v, lb, ub = _random_window(rng, n)
                lo_sum, hi_sum = lb.sum(), ub.sum()
                cap = float(rng.uniform(lo_sum - 2.0, hi_sum + 2.0)) if rep < 4 else float(lo_sum + (hi_sum - lo_sum) * rng.random())
                mu0 = 0.0 if rep % 2 == 0 else float(rng.uniform(-60.0, 60.0))
                miss = _mismatch(lib, v, lb, ub, cap, eq, mu0)
                modes.add(_fill(lib, v, lb, ub, cap, eq, mu0)[1].mode)
                if miss:
                    bad.append((n, eq, rep, miss[0]))
    return bad, modes


def test_random_windows_meet_the_twin():
    bad, modes = _sweep_failures(_lib())
    assert not bad, bad[:5]
    assert modes == {ROOT_FIND, AT_UB, AT_LB, NOTHING}   # the sweep reaches every mode


def _flat_start_case(n):
    """Half the periods far above their box, half far below: at the start m = 0 nobody is strictly inside (nf = 0)"""
    hi_n = (n + 1) // 2
    v = np.concatenate([np.full(hi_n, 10.0), np.full(n - hi_n, -10.0)])
    return v, np.zeros(n), np.ones(n), hi_n - 0.5


def _constructed_failures(lib):
    """The cases the sweep may miss, by construction; each is checked to BE the case it claims (mode, flags)"""
    bad, ran = [], set()

    def run(name, v, lb, ub, cap, eq, mu0, want_mode, **flags):
        ran.add(name)
        z, info = _fill(lib, v, lb, ub, cap, eq, mu0)
        if info.mode != want_mode or any(getattr(info, k) != w for k, w in flags.items()):
            bad.append((name, len(v), eq, "not the case it claims", vars(info)))
        miss = _mismatch(lib, v, lb, ub, cap, eq, mu0)
        if miss:
            bad.append((name, len(v), eq, miss[0]))
        return z, info

    rng = np.random.default_rng(7)
    for n in (1, 2, 15, 16, 17, 33, 48):
        v, lb, ub = _random_window(rng, n)
        s0 = float(np.clip(v, lb, ub).sum())
        # inactive row: the clipped point already satisfies it
        z, _ = run("inactive", v, lb, ub, s0 + 1.0, False, 3.0, NOTHING)
        if not np.array_equal(z, np.clip(v, lb, ub)):
            bad.append(("inactive", n, False, "moved"))
        run("inactive_eq", v, lb, ub, s0, True, 3.0, NOTHING)
        # a slack inequality beyond sum ub stays where the box puts it (NOT at ub)
        z, _ = run("slack_beyond_ub", v - 50.0, lb, ub, float(ub.sum()) + 1.0, False, 0.0, NOTHING)
        if not np.array_equal(z, np.clip(v - 50.0, lb, ub)):
            bad.append(("slack_beyond_ub", n, False, "moved"))
        # cap >= sum ub with equality: pinned at ub
        z, _ = run("pinned_ub", v - 50.0, lb, ub + 1.0, float((ub + 1.0).sum()) + 0.5, True, 0.0, AT_UB)
        if not np.array_equal(z, ub + 1.0):
            bad.append(("pinned_ub", n, True, "not ub"))
        # cap <= sum lb: pinned at lb, both kinds
        for eq in (False, True):
            z, _ = run("pinned_lb", v + 50.0, lb, ub + 1.0, float(lb.sum()) - 0.25, eq, 0.0, AT_LB)
            if not np.array_equal(z, lb):
                bad.append(("pinned_lb", n, eq, "not lb"))
        # a start on a flat piece: nf = 0, the step must bisect
        fv, flb, fub, fcap = _flat_start_case(n)
        for eq in (False, True):
            _, info = run("flat_start", fv, flb, fub, fcap, eq, 0.0, ROOT_FIND)
            if info.flat < 1:
                bad.append(("flat_start", n, eq, "no flat step", vars(info)))
        # an inequality whose bracket starts below zero (min (v - ub) < 0): the multiplier stays >= 0
        ub_w = np.maximum(ub, v + 5.0)
        lb_w = np.minimum(lb, ub_w)
        cap_w = float(lb_w.sum() + 0.5 * (np.clip(v, lb_w, ub_w).sum() - lb_w.sum()))
        if cap_w < float(np.clip(v, lb_w, ub_w).sum()) - 1e-9:
            run("bracket_below_zero", v, lb_w, ub_w, cap_w, False, 0.0, ROOT_FIND, lo_below_zero=True)
        # lb = ub on part of the window
        lbp = lb.copy()
        ubp = np.where(np.arange(n) % 2 == 0, lbp, lbp + 6.0)
        if n > 1:
            for eq in (False, True):
                run("fixed_periods", v + 10.0, lbp, ubp, float(lbp.sum() + 0.37 * (ubp.sum() - lbp.sum())), eq, 0.0, ROOT_FIND)
        # a warm multiplier outside the bracket, either side
        vv, ll, uu = v + 10.0, np.zeros(n), np.full(n, 20.0)
        capw = 0.4 * float(np.clip(vv, ll, uu).sum())
        for mu0 in (1e3, -1e3):
            run("warm_outside", vv, ll, uu, capw, True, mu0, ROOT_FIND, clamped=True)
        run("warm_outside", vv, ll, uu, capw, False, 1e3, ROOT_FIND, clamped=True)
    return bad, ran


CASES = {"inactive", "inactive_eq", "slack_beyond_ub", "pinned_ub", "pinned_lb", "flat_start", "bracket_below_zero", "fixed_periods",
         "warm_outside"}


def test_constructed_cases():
    bad, ran = _constructed_failures(_lib())
    assert not bad, bad[:5]
    assert ran == CASES


def test_each_mutation_fails():
    # without the bisection fallback a start on a flat piece never leaves it; with the pinned-at-ub mode open to
    # inequalities a slack row beyond sum ub is dragged up to ub
    for mutation, must_fail in (("MUT_NO_BISECT", "flat_start"), ("MUT_UB_FOR_INEQ", "slack_beyond_ub")):
        failed, _ = _constructed_failures(_lib(mutation))
        assert failed, mutation
        assert must_fail in {f[0] for f in failed}, (mutation, failed[:5])
        assert _sweep_failures(_lib(mutation))[0], mutation   # the random sweep sees it too


def test_infeasible_bounds_rule_on_both_sides_of_its_slack():
    lib = _lib()
    for cap in (0.25, 1000.0, -1000.0):
        slack = 64.0 * PROJ_TOL * max(1.0, abs(cap))
        for eq in (0, 1):
            assert lib.bounds_miss(cap + 2.0 * slack, cap + 10.0, cap, eq, PROJ_TOL) == 1      # sum lb beyond the capacity
            assert lib.bounds_miss(cap + 0.5 * slack, cap + 10.0, cap, eq, PROJ_TOL) == 0      # ... within the slack
            assert lib.bounds_miss(cap - 10.0, cap + 10.0, cap, eq, PROJ_TOL) == 0
        assert lib.bounds_miss(cap - 10.0, cap - 2.0 * slack, cap, 1, PROJ_TOL) == 1           # an equality sum ub cannot reach
        assert lib.bounds_miss(cap - 10.0, cap - 0.5 * slack, cap, 1, PROJ_TOL) == 0
        assert lib.bounds_miss(cap - 10.0, cap - 2.0 * slack, cap, 0, PROJ_TOL) == 0           # an inequality does not care


def _rule_rows(lib, zh, types, lims, peak_b, quad, pair_stride):
    """The site rows of one tile through site_row_z; the SOC scale is the caller's (here lim / sqrt, the stream kernel's)"""
    z = np.empty_like(zh)
    for r, ty in enumerate(types):
        for t in range(zh.shape[1]):
            scl = 1.0
            if ty in (SOC_RE, SOC_IM):
                rr = r if ty == SOC_RE else r - pair_stride
                n2 = zh[rr, t] ** 2 + zh[rr + pair_stride, t] ** 2
                if n2 > lims[rr] * lims[rr]:
                    scl = lims[rr] / math.sqrt(n2)
            z[r, t] = lib.site_z(ty, zh[r, t], lims[r], peak_b[t], quad, scl)
    return z


def test_site_row_step_against_the_twin():
    lib = _lib()
    rng = np.random.default_rng(11)
    T, rho, lf = 7, 0.3, 0.8
    peak_b = np.array([2.0, BIG, 0.5, 1.0, BIG, 3.0, 0.1])
    # SOC site: M discs (re rows, then im rows), the load-flattening row, the peak row
    M = 3
    limits = np.array([1.0, 2.5, 0.2])
    zh = rng.uniform(-3.0, 3.0, (2 * M + 2, T))
    site = SimpleNamespace(M=M, cone=admm_ref.CONE_SOC, has_flat=True, has_peak=True)
    want = admm_ref._prox_rows(zh, rho, site, limits, peak_b, T, lf, None)
    got = _rule_rows(lib, zh, [SOC_RE] * M + [SOC_IM] * M + [QUAD, PEAK], list(limits) * 2 + [0.0, 0.0], peak_b, rho / (rho + lf), M)
    # sqrt(re^2 + im^2) against hypot: a few units in the last place of the scale, nothing more
    assert np.allclose(got, want, rtol=8 * np.finfo(float).eps, atol=0.0)
    assert np.array_equal(got[2 * M:], want[2 * M:])                      # prox and peak rows: the same operations
    inside = np.hypot(zh[:M], zh[M:2 * M]) <= limits[:, None]
    assert inside.any() and not inside.all()
    assert np.array_equal(got[:M][inside], zh[:M][inside])                # a point inside its disc does not move
    # linear site: box rows and the peak row
    zh = rng.uniform(-3.0, 3.0, (M + 1, T))
    site = SimpleNamespace(M=M, cone=admm_ref.CONE_LINEAR, has_flat=False, has_peak=True)
    want = admm_ref._prox_rows(zh, rho, site, limits, peak_b, T, 0.0, None)
    got = _rule_rows(lib, zh, [BOX] * M + [PEAK], list(limits) + [0.0], peak_b, 1.0, 0)
    assert np.array_equal(got, want)
    # padding rows and the demand-charge row pass through: the horizon-wide prox follows in the kernels
    for ty in (FREE, MAX):
        assert lib.site_z(ty, 1.75, 0.5, 0.5, 0.5, 0.5) == 1.75


def _exact_tau(zv, cw):
    """root of sum (z - tau)+ = cw from the sorted values"""
    s = np.sort(zv)[::-1]
    for k in range(1, len(s) + 1):
        tau = (s[:k].sum() - cw) / k
        if k == len(s) or tau >= s[k]:
            return tau


def test_demand_charge_tau():
    lib = _lib()
    rng = np.random.default_rng(5)
    for n in (1, 2, 16, 17, 48, 144):
        for cw in (1e-3, 0.7, 40.0, 1e4):
            zv = np.ascontiguousarray(rng.uniform(-5.0, 30.0, n))
            tau = D(0.0)
            steps = lib.dc_tau(n, _ptr(zv), cw, PROJ_TOL, 200, ctypes.byref(tau))
            assert steps <= n + 2   # Newton on a convex piecewise-linear function from the left: monotone, one piece per step
            assert abs(np.maximum(zv - tau.value, 0.0).sum() - cw) <= 16.0 * PROJ_TOL * max(1.0, cw) * 2, (n, cw)
            assert math.isclose(tau.value, _exact_tau(zv, cw), rel_tol=0.0, abs_tol=1e-12 * max(1.0, cw, np.abs(zv).max()))
    # the guard is the caller's: beyond guard_max steps the search stops where it is
    zv = np.ascontiguousarray(np.arange(48, dtype=float))
    tau = D(0.0)
    assert lib.dc_tau(48, _ptr(zv), 500.0, PROJ_TOL, 0, ctypes.byref(tau)) == 1 and tau.value == 47.0 - 500.0
    assert lib.dc_tau(48, _ptr(zv), 500.0, PROJ_TOL, 2, ctypes.byref(tau)) == 3
