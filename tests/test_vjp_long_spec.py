"""tests/vjp_spec.py beyond horizon 32 (the shapes of vjp_long_kernel, adacharge_amd/csrc/acn_qp_vjp_long.hpp), on the CPU:
the pools of tests/polish_long_cases.py are fit for holding the kernel to the specification (tests/test_vjp_long_gpu.py
does that, with ``long_points`` of this file), and the specification itself matches central finite differences taken
through the polish's specification at horizons 33 ... 48, with the row tables of both raised to the worst case of the
shape as the long kernels' are."""
import functools

import numpy as np
import pytest

from adacharge_amd import backend
from tests import polish_long_cases as PLC
from tests import vjp_spec as VS
from tests.test_vjp_spec import FD_TOL, STEP, directions, moved, rel_err

# The problems of the finite-difference test, chosen among the full-rank ones without a weak member (ct54_t48[1, 3, 4],
# b52_t48_two[0, 1, 2]) as the first of each pool whose working set stays the same INSIDE the step of 1e-4 in all three
# directions.  Measured with this file, worst per problem: ct54_t48[3] 2.3e-8 (one site limit), b52_t48_two[0] 3.0e-8
# (random dq).  Not chosen: b52_t48_two[1] and [2] take another working set at one perturbed point of dq; ct54_t48[1] takes
# the same set at both perturbed points of `caps`, but the polish needs 20 rounds to the upper one -- a constraint joins and
# leaves on the way -- and the difference is 2.1e-3 at step 1e-4 against 1.2e-8 at step 1e-5: a kink inside the step, which
# the end points' working sets do not show.
FD_PROBLEMS = (("ct54_t48", 3), ("b52_t48_two", 0))


@functools.lru_cache(maxsize=None)
def long_points(name):
    """(batch, x, y, status) of a pool: the polish specification's certified point from the twin's answer where the twin
    ends SOLVED (status 1); zeros and status MAX_ITER elsewhere (an infeasible problem)"""
    batch, sol = PLC.pool(name), PLC.twin(name)
    todo = [b for b in range(batch.B) if sol["status"][b] == 1]
    res = PLC.spec_many([PLC.spec_job(batch, b, sol["x"][b], sol["y"][b]) for b in todo])
    x, y = np.zeros((batch.B, batch.N, batch.Tm)), np.zeros((batch.B, batch.site.Mg, batch.Tm))
    status = np.full(batch.B, backend.STATUS_MAX_ITER, np.int32)
    for b, (xb, info) in zip(todo, res):
        assert info["ok"], (name, b, info["why"])   # every problem the twin ends SOLVED is certified
        T = xb.shape[1]
        x[b, :, :T], y[b, :, :T], status[b] = xb, info["y"], 1
    for a in (x, y, status):
        a.setflags(write=False)
    return batch, x, y, status


def long_weights(shape):
    return np.random.default_rng(5).standard_normal(shape)


@functools.lru_cache(maxsize=None)
def long_ref(name):
    """the specification on every problem of a pool at ``long_points``, g = long_weights: (stacked outputs, per problem)"""
    batch, x, y, status = long_points(name)
    return VS.vjp_batch(batch, x, y, long_weights(x.shape), status, max_rows=PLC.worst_rows(batch.site, batch.Tm))


@pytest.mark.parametrize("name", list(PLC.POOLS))
def test_the_pools_are_fit(name):
    batch, x, y, status = long_points(name)
    solved = PLC.twin(name)["status"] == 1
    assert (status[solved] == 1).all() and solved.sum() >= 2
    ref, each = long_ref(name)
    assert (ref["info"][solved, 0] == VS.DONE).all(), ref["info"]
    assert (ref["info"][~solved, 0] == VS.BAD_STATUS).all()
    rows = ref["info"][:, 1]
    print(f"[vjp-long] {name}: Tm {batch.Tm} rows {rows.tolist()} rank / rows of C {[(e['rank'], e['rows_c']) for e in each]}")
    assert rows.max() > 256 or batch.Tm <= 49, (name, rows)   # beyond the short kernel's row tables, or a horizon it nearly reaches
    if name == "n8_t144":
        assert all(e["rank"] < e["rows_c"] for e in each)     # dependent tight rows on every problem
    if name == "ct54_t48":
        assert all(e["rank"] == e["rows_c"] for e in each)
    if name == "n64_lin_t96_peak":
        assert PLC.twin(name)["status"][3] == 3 and status[3] == backend.STATUS_MAX_ITER   # the infeasible fourth


def _at(batch, xp, info):
    """a polished point padded to the batch's shape"""
    x, y = np.zeros((batch.N, batch.Tm)), np.zeros((batch.site.Mg, batch.Tm))
    T = xp.shape[1]
    x[:, :T], y[:, :T] = xp, info["y"]
    return x, y


@pytest.mark.parametrize("name,b", FD_PROBLEMS, ids=lambda v: str(v))
def test_specification_matches_central_differences_beyond_horizon_32(name, b):
    full, xs, ys, _ = long_points(name)
    batch, x, y = full.subset(slice(b, b + 1)), xs[b], ys[b]
    assert int(batch.T[0]) > 32
    max_rows = PLC.worst_rows(batch.site, batch.Tm)
    g = np.random.default_rng(11).standard_normal((batch.N, batch.Tm))
    s = VS.vjp(batch, 0, x, y, g, max_rows=max_rows)
    assert s["info"][0] == VS.DONE and s["info"][2] == 0, s["info"]   # no weak member: the map is differentiable here
    assert s["rank"] == s["rows_c"] > 0                                 # no dependent tight row
    assert s["res"][0] <= 1e-12 and s["res"][1] <= 1e-8, s["res"]
    dirs = directions(batch, s)
    perturbed = []
    for _, arr, d, _ in dirs:
        base = batch.site.limits if arr == "limits" else getattr(batch, arr)
        perturbed += [moved(batch, **{arr: base + sign * STEP * d}) for sign in (1.0, -1.0)]
    res = PLC.spec_many([PLC.spec_job(mb, 0, x, y) for mb in perturbed])   # (the polish's specification, MAX_ROWS raised)
    for k, (dname, _, _, pred) in enumerate(dirs):
        vals = []
        for mb, (xp, info) in zip(perturbed[2 * k: 2 * k + 2], res[2 * k: 2 * k + 2]):
            assert info["ok"], (name, b, dname, info["why"])
            xx, yy = _at(mb, xp, info)
            vals.append(float((g * xx).sum()))
            assert VS.vjp(mb, 0, xx, yy, g, max_rows=max_rows)["ws"] == s["ws"], (name, b, dname, "the working set changes inside the step")
        fd = (vals[0] - vals[1]) / (2 * STEP)
        err = rel_err(fd, pred)
        print(f"[vjp-long] {name}[{b}] {dname}: fd {fd:.9e} adjoint {pred:.9e} rel {err:.2e}")
        assert abs(pred) > 1e-6, (name, b, dname, pred)   # (the comparison is not between zeros)
        assert err <= FD_TOL, (name, b, dname, fd, pred, err)


def test_switch_is_declared_and_refuses_a_null_handle(hip_library):
    assert "acnqp_set_long_vjp" in backend.EXPORTED_SYMBOLS
    assert hip_library.acnqp_abi_version() == 10
    assert hip_library.acnqp_set_long_vjp(None, 1) == -1
    assert b"acnqp_set_long_vjp: null handle" in hip_library.acnqp_last_error()
