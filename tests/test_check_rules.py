"""The residual-check rules of adacharge_amd/csrc/acn_qp_check.hpp -- the ONE copy all five solver kernels call --
compiled for the host (g++, as oracle/build.py compiles the C twin) and pinned branch by branch.  The expected values
are written out here from oracle/admm_port.c's statement of the same rules (its certificate, stall rule and rho update),
not computed by the header.  Three mutations (applied by a -D of the shim below, never by the header) must each make the
truth table fail: the peak sign tests flipped, `bad` never set, the SOC term dropped."""
import ctypes
import functools
import math
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adacharge_amd", "csrc")

SHIM = r"""
#define __host__
#define __device__
#include "acn_qp_check.hpp"
using namespace acnqp;
extern "C" {
void row_ray(int ty, double v, double vi, double lim, double peak, double big, double vtol, double* ssum, double* bad) {
#ifdef MUT_PEAK_SIGN
  if (ty == kRowPeak) v = -v;
#endif
#ifdef MUT_NO_SOC
  if (ty == kRowSocRe) ty = kRowSocIm;
#endif
#ifdef MUT_NO_BAD
  double unused = 0;
  cert_row_ray<double>(ty, v, vi, cert_row_has_limit(ty) ? lim : 0.0, peak, big, vtol, *ssum, unused);
#else
  cert_row_ray<double>(ty, v, vi, cert_row_has_limit(ty) ? lim : 0.0, peak, big, vtol, *ssum, *bad);
#endif
}
int gate(double vn, double atv, double qnorm, double* vtol) { return cert_gate<double>(vn, atv, qnorm, *vtol); }
int verdict(double bad_max, double stot, double vtol) { return cert_verdict<double>(bad_max, stot, vtol); }
double candidate(double l, int eq) { return cert_session_candidate<double>(l, eq != 0); }
double support_term(double ub, double lb, double dv) { return cert_support_term<double>(ub, lb, dv); }
int is_converged(double eps_abs, double eps_rel, double pri, double dua, double npri, double ndua, double* eps_p, double* eps_d) {
  const CheckTol<double> e = check_tolerances<double>(eps_abs, eps_rel, npri, ndua);
  *eps_p = e.eps_p; *eps_d = e.eps_d;
  return converged(pri, dua, e);
}
double score(double pri, double dua, double eps_p, double eps_d) { return stall_score<double>(pri, dua, CheckTol<double>{eps_p, eps_d}); }
int improved(double s, double best) { return stall_improved<double>(s, best); }
int reached(int stall_iters, int it, int best_it, double s, double best) { return stall_reached<double>(stall_iters, it, best_it, s, best); }
double rho_update(double pri, double dua, double npri, double ndua, double adapt_tol, int n_adapt, double rho) {   // -1: keep
  const double ratio = rho_ratio<double>(pri, dua, npri, ndua);
  return rho_outside_band(ratio, adapt_tol, n_adapt) ? rho_clamped<double>(rho * ratio) : -1.0;
}
double row_weight(int ty, double yr, double yi, double ytol, int live) { return polish_row_weight<double>(ty, yr, yi, ytol, live != 0); }
double ytol_of(double qnorm) { return polish_ytol<double>(qnorm); }
int fits(double cnt, int pol_rows) { return polish_fits<double>(cnt, pol_rows); }
}
"""

D = ctypes.c_double
FREE, BOX, SOC_RE, SOC_IM, PEAK, QUAD, MAX = 0, 1, 2, 3, 4, 5, 6   # row types (acn_qp_check.hpp, oracle/admm_port.c)
BIG = 1e300


@functools.lru_cache(maxsize=None)
def _lib(mutation=""):
    tmp = tempfile.mkdtemp(prefix="acnqp_check_")
    src, so = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "shim" + (mutation or "plain") + ".so")
    with open(src, "w") as f:
        f.write(SHIM)
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.run([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, *(["-D" + mutation] if mutation else []), src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    shutil.rmtree(tmp)   # (the mapping stays; nothing built is left behind)
    P = ctypes.POINTER(D)
    for name, res, args in (("row_ray", None, [ctypes.c_int, D, D, D, D, D, D, P, P]), ("gate", ctypes.c_int, [D, D, D, P]),
                            ("verdict", ctypes.c_int, [D, D, D]), ("candidate", D, [D, ctypes.c_int]), ("support_term", D, [D, D, D]),
                            ("is_converged", ctypes.c_int, [D, D, D, D, D, D, P, P]), ("score", D, [D, D, D, D]),
                            ("improved", ctypes.c_int, [D, D]), ("reached", ctypes.c_int, [ctypes.c_int] * 3 + [D, D]),
                            ("rho_update", D, [D, D, D, D, D, ctypes.c_int, D]), ("row_weight", D, [ctypes.c_int, D, D, D, ctypes.c_int]),
                            ("ytol_of", D, [D]), ("fits", ctypes.c_int, [D, ctypes.c_int])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


VTOL, LIM, PEAK_LIM, VI = 0.5, 3.0, 7.0, 0.75
VS = (-2 * VTOL, -VTOL / 2, 0.0, VTOL / 2, 2 * VTOL)


def _expected_ray(ty, v, peak):
    """(ssum, bad) of one row, as oracle/admm_port.c states the ladder"""
    if ty == BOX:
        return LIM * max(v, 0.0), float(v < -VTOL)
    if ty == PEAK:
        if peak < BIG:
            return PEAK_LIM * max(v, 0.0), float(v < -VTOL)
        return 0.0, float(v > VTOL or v < -VTOL)
    if ty == SOC_RE:
        return LIM * math.sqrt(v * v + VI * VI), 0.0
    if ty == SOC_IM:
        return 0.0, 0.0
    return 0.0, float(abs(v) > VTOL)   # free / prox rows admit no ray


def _ray_failures(lib):
    bad_cases = []
    for ty in (FREE, BOX, SOC_RE, SOC_IM, PEAK, QUAD, MAX):
        for v in VS:
            for peak in (PEAK_LIM, BIG):
                ssum, bad = D(0.25), D(0.0)   # ssum accumulates on what it holds
                lib.row_ray(ty, v, VI, LIM, peak, BIG, VTOL, ctypes.byref(ssum), ctypes.byref(bad))
                es, eb = _expected_ray(ty, v, peak)
                if not (math.isclose(ssum.value, 0.25 + es, rel_tol=1e-15, abs_tol=0.0) and bad.value == eb):
                    bad_cases.append((ty, v, peak, ssum.value, bad.value, 0.25 + es, eb))
    return bad_cases


def test_row_ray_truth_table():
    assert not _ray_failures(_lib())


def test_row_ray_leaves_a_set_bad_flag_alone():
    lib = _lib()
    for ty in (FREE, BOX, SOC_RE, SOC_IM, PEAK, QUAD, MAX):
        ssum, bad = D(0.0), D(1.0)
        lib.row_ray(ty, 0.0, 0.0, LIM, PEAK_LIM, BIG, VTOL, ctypes.byref(ssum), ctypes.byref(bad))
        assert bad.value == 1.0, ty


def test_each_mutation_fails_the_truth_table():
    for mutation, rows in (("MUT_PEAK_SIGN", {PEAK}), ("MUT_NO_BAD", {FREE, BOX, PEAK, QUAD, MAX}), ("MUT_NO_SOC", {SOC_RE})):
        failed = _ray_failures(_lib(mutation))
        assert failed, mutation
        assert {f[0] for f in failed} == rows, (mutation, failed)


def test_gate_and_verdict():
    lib = _lib()
    vtol = D(0.0)
    assert lib.gate(2.0, 1e-4, 1.0, ctypes.byref(vtol)) == 1 and vtol.value == 1e-4 * 2.0
    assert lib.gate(2.0, 2e-4, 1.0, ctypes.byref(vtol)) == 1      # |A'v| <= vtol, equality included
    assert lib.gate(2.0, 3e-4, 1.0, ctypes.byref(vtol)) == 0      # A'v is not ~ 0
    assert lib.gate(1e-13, 0.0, 1.0, ctypes.byref(vtol)) == 0     # |v| <= 1e-12 max(1, |q|): no direction
    assert lib.gate(5e-10, 0.0, 1e3, ctypes.byref(vtol)) == 0     # ... scaled by |q| = 1e3
    assert lib.gate(2e-9, 0.0, 1e3, ctypes.byref(vtol)) == 1
    assert lib.gate(2e-12, 0.0, 0.5, ctypes.byref(vtol)) == 1     # max(1, |q|) = 1
    assert lib.verdict(0.0, -1.0, 0.5) == 1
    assert lib.verdict(1.0, -1.0, 0.5) == 0      # a row admits no ray
    assert lib.verdict(0.0, -0.5, 0.5) == 0      # strictly below -vtol
    assert lib.verdict(0.0, -0.4, 0.5) == 0
    assert lib.verdict(0.0, 1.0, 0.5) == 0


def test_session_support_terms():
    lib = _lib()
    assert lib.candidate(-1.0, 1) == -1.0 and lib.candidate(-1.0, 0) == 0.0 and lib.candidate(2.0, 0) == 2.0 and lib.candidate(2.0, 1) == 2.0
    assert lib.support_term(3.0, 1.0, 2.0) == 6.0     # ub (dv)+
    assert lib.support_term(3.0, 1.0, -2.0) == -2.0   # lb (dv)-
    assert lib.support_term(3.0, 1.0, 0.0) == 0.0


def test_convergence_and_stall_rule():
    lib = _lib()
    ep, ed = D(0.0), D(0.0)
    assert lib.is_converged(1e-3, 1e-2, 0.1, 0.2, 10.0, 20.0, ctypes.byref(ep), ctypes.byref(ed)) == 1
    assert ep.value == 1e-3 + 1e-2 * 10.0 and ed.value == 1e-3 + 1e-2 * 20.0
    assert lib.is_converged(1e-3, 1e-2, 0.102, 0.2, 10.0, 20.0, ctypes.byref(ep), ctypes.byref(ed)) == 0   # primal alone
    assert lib.is_converged(1e-3, 1e-2, 0.1, 0.202, 10.0, 20.0, ctypes.byref(ep), ctypes.byref(ed)) == 0   # dual alone
    assert lib.score(2.0, 3.0, 1.0, 2.0) == 2.0 and lib.score(1.0, 3.0, 1.0, 2.0) == 1.5
    assert lib.score(1.0, 0.0, 0.0, 1.0) == 1.0 / 1e-300           # eps floored at 1e-300
    assert lib.improved(0.89, 1.0) == 1 and lib.improved(0.9, 1.0) == 0 and lib.improved(0.95, 1.0) == 0   # 10 % better, strictly
    assert lib.reached(100, 250, 100, 1.2, 1.0) == 1
    assert lib.reached(100, 200, 100, 1.25, 1.0) == 1             # the window and kStallNear = 1.25, both inclusive
    assert lib.reached(100, 199, 100, 1.2, 1.0) == 0              # window not over
    assert lib.reached(100, 250, 100, 1.26, 1.0) == 0             # in the transient after a rho change, not on the plateau
    assert lib.reached(0, 250, 100, 1.0, 1.0) == 0                # stall_iters = 0: off


def test_rho_adaptation():
    lib = _lib()
    keep = -1.0
    assert lib.rho_update(4.0, 1.0, 1.0, 1.0, 5.0, 0, 0.1) == keep            # ratio 2: inside [1/5, 5]
    assert lib.rho_update(0.25, 1.0, 1.0, 1.0, 5.0, 0, 0.1) == keep           # ratio 1/2
    assert math.isclose(lib.rho_update(100.0, 1.0, 1.0, 1.0, 5.0, 0, 0.1), 1.0, rel_tol=1e-15)    # ratio 10: rho * 10
    assert math.isclose(lib.rho_update(1.0, 100.0, 1.0, 1.0, 5.0, 0, 0.1), 0.01, rel_tol=1e-15)   # ratio 1/10
    assert math.isclose(lib.rho_update(144.0, 1.0, 4.0, 1.0, 5.0, 0, 0.1), 0.6, rel_tol=1e-15)    # relative residuals: ratio 6
    assert lib.rho_update(100.0, 1.0, 4.0, 1.0, 5.0, 0, 0.1) == keep          # ratio 5 is still inside (strict)
    assert lib.rho_update(1.0, 100.0, 1.0, 4.0, 5.0, 0, 0.1) == keep          # ratio 1/5 too
    assert lib.rho_update(1e6, 1.0, 1.0, 1.0, 5.0, 0, 1e5) == 1e6             # clamps
    assert lib.rho_update(1.0, 1e6, 1.0, 1.0, 5.0, 0, 1e-5) == 1e-6
    assert lib.rho_update(36.0, 1.0, 1.0, 1.0, 5.0, 0, 1.0) == 6.0            # ratio 6 leaves the band 5 ...
    assert lib.rho_update(36.0, 1.0, 1.0, 1.0, 5.0, 2, 1.0) == keep           # ... but not 5 (1 + 2 / 8) = 6.25
    assert lib.rho_update(81.0, 1.0, 1.0, 1.0, 5.0, 8, 1.0) == keep           # 5 (1 + 8 / 8) = 10
    assert lib.rho_update(1.0, 64.0, 1.0, 1.0, 5.0, 8, 1.0) == keep           # 1 / 8 > 1 / 10
    assert lib.rho_update(1.0, 64.0, 1.0, 1.0, 5.0, 0, 1.0) == 0.125
    assert lib.rho_update(4.0, 0.0, 1.0, 0.0, 5.0, 0, 1.0) == 1e6             # floors 1e-12 / 1e-30 of the denominators


def test_polish_row_weight():
    lib = _lib()
    assert lib.row_weight(BOX, 1.0, 0.0, 0.5, 1) == 1.0 and lib.row_weight(PEAK, 1.0, 0.0, 0.5, 1) == 1.0
    assert lib.row_weight(BOX, 1.0, 0.0, 0.5, 0) == 0.0            # the row's period does not exist
    assert lib.row_weight(BOX, 0.5, 0.0, 0.5, 1) == 0.0            # strictly above ytol
    assert lib.row_weight(BOX, -1.0, 0.0, 0.5, 1) == 0.0
    assert lib.row_weight(SOC_RE, 0.3, 0.4, 0.45, 1) == 2.0        # |(0.3, 0.4)| = 0.5: normal + tangent
    assert lib.row_weight(SOC_RE, 0.3, 0.4, 0.6, 1) == 0.0
    assert lib.row_weight(SOC_RE, -0.3, -0.4, 0.45, 1) == 2.0
    for ty in (FREE, SOC_IM, QUAD, MAX):
        assert lib.row_weight(ty, 1.0, 1.0, 0.5, 1) == 0.0, ty
    assert lib.ytol_of(0.5) == 1e-9 and lib.ytol_of(1e3) == 1e-9 * 1e3
    assert lib.fits(10.0, 18) == 1 and lib.fits(11.0, 18) == 0     # eight rows of headroom
