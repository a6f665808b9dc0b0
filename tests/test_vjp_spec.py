"""tests/vjp_spec.py, the numpy specification of the gradients through the solve, held to central finite differences taken
through the polish's specification (oracle/polish_ref.polish_batch_problem), and its rules by hand.  CPU only; the kernel
is held to the specification in tests/test_vjp_gpu.py."""
import copy
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

from adacharge_amd import backend
from oracle.polish_ref import polish_batch_problem
from tests import helpers as H
from tests import vjp_spec as VS
from tests.test_duals_spec import ipm_energy_duals

STEP = 1e-4
# |finite difference - adjoint| / max(|finite difference|, |adjoint|) of a directional derivative at step 1e-4: 1e-7, set
# when the feature was specified as ten times the worst error of a first measurement (9e-9, all caps moved together).  The
# central difference through a polish that stops at a step of 1e-7 A limits it, not the adjoint.  Measured with this file
# over c01, c05, c09, c06, c07, worst per quantity: random dq 2.6e-11 (c05), all caps 2.2e-8 (c01), one site limit
# 7.7e-9 (c01); c00's dq 6.8e-12.
FD_TOL = 1e-7
FD_CASES = ("c01", "c05", "c09", "c06", "c07")


@functools.lru_cache(maxsize=None)
def certified(key):
    """(batch, x, y) of a golden case: the IPM's point polished by the specification -- a KKT point to 1e-8"""
    g = H.load_golden()
    infra, iface = H.caltech_interface()
    sl, meta, _ = H.golden_case(g, key)
    batch, x0, y0, _ = ipm_energy_duals(sl, infra, iface, meta)
    x, info = polish_batch_problem(batch, 0, x0, y0)
    assert info["ok"], (key, info["why"])
    xx, yy = np.zeros((batch.N, batch.Tm)), np.zeros((batch.site.Mg, batch.Tm))
    xx[:, :x.shape[1]], yy[:, :x.shape[1]] = x, info["y"]
    return batch, xx, yy


def weights(batch, seed):
    return np.random.default_rng(seed).standard_normal((batch.N, batch.Tm))


def moved(batch, **arrays):
    """a copy of the batch with some arrays (or the site's limits) replaced"""
    out = copy.copy(batch)
    for k, v in arrays.items():
        if k == "limits":
            out.site = dataclasses.replace(batch.site, limits=v)
        else:
            setattr(out, k, v)
    return out


def central_difference(batch, x, y, g, name, direction):
    """d/dh of <g, x*(theta + h direction)> through the polish's specification, started at (x, y); and the working sets the
    adjoint's specification takes at the two perturbed optima"""
    vals, sets = [], []
    for sign in (1.0, -1.0):
        base = batch.site.limits if name == "limits" else getattr(batch, name)
        mb = moved(batch, **{name: base + sign * STEP * direction})
        xp, info = polish_batch_problem(mb, 0, x, y)
        assert info["ok"], (name, sign, info["why"])
        T = xp.shape[1]
        vals.append(float((g[:, :T] * xp).sum()))
        xx, yy = np.zeros_like(x), np.zeros_like(y)
        xx[:, :T], yy[:, :T] = xp, info["y"]
        sets.append(VS.vjp(mb, 0, xx, yy, g)["ws"])
    return (vals[0] - vals[1]) / (2 * STEP), sets


def rel_err(fd, pred):
    return abs(fd - pred) / max(abs(fd), abs(pred), 1e-300)


def directions(batch, s):
    """(name, array name, direction, the adjoint's prediction) of the three directional derivatives"""
    rng = np.random.default_rng(7)
    dq = rng.standard_normal(batch.q.shape)
    dq[0][:, int(batch.T[0]):] = 0.0
    dcap = (batch.s_len > 0).astype(float)
    r = int(np.argmax((s["grow"][: batch.site.M] != 0).sum(axis=1)))
    dlim = np.zeros(batch.site.M)
    dlim[r] = 1.0
    return (("dq", "q", dq, float((s["gq"] * dq[0]).sum())),
            ("caps", "s_cap", dcap, float((s["gcap"] * dcap[0]).sum())),
            ("limit", "limits", dlim, float(s["grow"][r].sum())))


@pytest.mark.parametrize("key", FD_CASES)
def test_specification_matches_central_differences(key):
    batch, x, y = certified(key)
    g = weights(batch, 11)
    s = VS.vjp(batch, 0, x, y, g)
    assert s["info"][0] == VS.DONE and s["info"][2] == 0, s["info"]          # no weak member: the map is differentiable here
    assert s["rank"] == s["rows_c"] > 0                                        # no dependent tight row
    assert s["res"][0] <= 1e-12 and s["res"][1] <= 1e-8, s["res"]
    for name, arr, d, pred in directions(batch, s):
        fd, sets = central_difference(batch, x, y, g, arr, d)
        assert sets[0] == sets[1] == s["ws"], (key, name, "the working set changes inside the step")
        err = rel_err(fd, pred)
        print(f"[vjp] {key} {name}: fd {fd:.9e} adjoint {pred:.9e} rel {err:.2e}")
        assert abs(pred) > 1e-6, (key, name, pred)   # (the comparison is not between zeros)
        assert err <= FD_TOL, (key, name, fd, pred, err)


def test_dependent_row_keeps_gq_and_reproduces_g():
    """c00: one tight row depends on the others (rank 28 of 29) and one bound is weakly active.  dL/dq is unique and still
    matches finite differences; the rows' gradients are the least-norm ones, only required to reproduce g through C'm."""
    batch, x, y = certified("c00")
    g = weights(batch, 11)
    s = VS.vjp(batch, 0, x, y, g)
    assert s["info"][0] == VS.DONE
    assert s["rank"] == s["rows_c"] - 1, (s["rank"], s["rows_c"])
    assert s["info"][2] == 1, s["info"]
    name, arr, d, pred = directions(batch, s)[0]
    fd, _ = central_difference(batch, x, y, g, arr, d)
    print(f"[vjp] c00 dq: fd {fd:.9e} adjoint {pred:.9e} rel {rel_err(fd, pred):.2e}")
    assert rel_err(fd, pred) <= FD_TOL
    assert s["res"][0] <= 1e-9, s["res"]   # H a + C'm = g on the free variables, whatever m the dependent rows share


def test_exact_zeros_where_promised():
    batch, x, y = certified("c06")
    s = VS.vjp(batch, 0, x, y, weights(batch, 3))
    T = int(batch.T[0])
    lb, ub = batch.lb[0], np.maximum(batch.ub[0], batch.lb[0])
    on_bound = (x <= lb + 1e-7) | (x >= ub - 1e-7)
    window = np.zeros_like(on_bound)
    for k in range(batch.K):
        for i in range(batch.N):
            window[i, batch.s_off[0, k, i]: batch.s_off[0, k, i] + batch.s_len[0, k, i]] = True
    assert (s["gq"][on_bound | ~window] == 0).all() and (s["gq"][:, T:] == 0).all()
    assert (s["gq"][~on_bound] != 0).any()
    assert (s["gcap"][batch.s_len[0] == 0] == 0).all()
    sums = np.array([[x[i, batch.s_off[0, k, i]: batch.s_off[0, k, i] + batch.s_len[0, k, i]].sum() for i in range(batch.N)] for k in range(batch.K)])
    assert (s["gcap"][sums < batch.s_cap[0] - 1e-3] == 0).all()   # slack energy rows
    M = batch.site.M
    assert (s["grow"][np.hypot(y[:M], y[M:2 * M]) == 0] == 0).all() and (s["grow"] != 0).any()
    assert (s["glb"][~(x <= lb + 1e-7)] == 0).all() and (s["gub"][~(x >= ub - 1e-7)] == 0).all()
    assert ((s["glb"] != 0) & (s["gub"] != 0)).sum() == 0


def test_unsolved_problem_gets_zeros_and_verdict_1():
    batch, x, y = certified("c01")
    s = VS.vjp(batch, 0, x, y, weights(batch, 3), status=backend.STATUS_MAX_ITER)
    assert s["info"].tolist() == [VS.BAD_STATUS, 0, 0, 0]
    assert all((s[k] == 0).all() for k in VS.OUTPUTS)
    assert VS.vjp(batch, 0, x, y, weights(batch, 3), status=backend.STATUS_SOLVED_INACCURATE)["info"][0] == VS.DONE


def test_working_set_beyond_the_row_tables_gets_zeros_and_verdict_2():
    batch, x, y = certified("c06")
    full = VS.vjp(batch, 0, x, y, weights(batch, 3))
    s = VS.vjp(batch, 0, x, y, weights(batch, 3), max_rows=int(full["info"][1]) - 1)
    assert s["info"].tolist() == [VS.ROWS, 0, 0, 0] and all((s[k] == 0).all() for k in VS.OUTPUTS)


def test_equality_energy_rows_are_all_tight():
    """with s_eq every energy row is a row of C, slack or not: the schedule's energy cannot move, so dL/dq sums to zero over
    every window with a free variable, and an equality row is never a weak member"""
    batch, x, y = certified("c01")
    sums = np.array([[[x[i, batch.s_off[0, k, i]: batch.s_off[0, k, i] + batch.s_len[0, k, i]].sum() for i in range(batch.N)]
                      for k in range(batch.K)]])
    eqb = moved(batch, s_eq=np.ones(1, np.uint8), s_cap=np.where(batch.s_len > 0, sums, batch.s_cap))
    g = weights(batch, 5)
    s, base = VS.vjp(eqb, 0, x, y, g), VS.vjp(batch, 0, x, y, g)
    assert s["info"][0] == VS.DONE and s["info"][2] == 0
    seen = 0
    for k in range(batch.K):
        for i in range(batch.N):
            o, L = int(batch.s_off[0, k, i]), int(batch.s_len[0, k, i])
            if L and (s["gq"][i, o:o + L] != 0).any():
                assert abs(s["gq"][i, o:o + L].sum()) <= 1e-12 * np.abs(s["gq"]).max()
                seen += 1
    # rows that were slack as inequalities are rows of C now (a window with ONE free variable pins it: gq 0, gcap not)
    assert (s["gcap"] != 0).sum() >= seen > (base["gcap"] != 0).sum()


def test_weak_member_is_counted():
    """a bound moved onto a free variable's value: the variable is fixed there with a zero multiplier"""
    batch, x, y = certified("c01")
    g = weights(batch, 5)
    base = VS.vjp(batch, 0, x, y, g)
    lb, ub = batch.lb[0], np.maximum(batch.ub[0], batch.lb[0])
    i, t = np.argwhere((x > lb + 1.0) & (x < ub - 1.0))[0]
    lb2 = batch.lb.copy()
    lb2[0, i, t] = x[i, t]
    s = VS.vjp(moved(batch, lb=lb2), 0, x, y, g)
    assert base["info"][2] == 0 and s["info"][2] == 1
    assert s["info"][3] == base["info"][3] - 1 and s["gq"][i, t] == 0


def test_entries_are_declared_and_refuse_a_null_handle(hip_library):
    assert {"acnqp_vjp_host", "acnqp_vjp_device"} <= set(backend.EXPORTED_SYMBOLS)
    assert hip_library.acnqp_abi_version() == 10
    assert hip_library.acnqp_vjp_host(*[None] * 14) == -1
    assert b"null handle" in hip_library.acnqp_last_error()
    assert hip_library.acnqp_vjp_device(*[None] * 15) == -1
    assert b"acnqp_vjp_device: null handle" in hip_library.acnqp_last_error()
