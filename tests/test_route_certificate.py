"""Every kernel route's answers, certified by the host KKT check (oracle/kkt.py) with the constants the C twin set.

A problem padded to another t_max, or given empty session slots, is the same problem (include/acn_qp.h: periods
t >= horizon[b] are dead) but runs on another kernel family: acnqp_route decides on (t_max, k_sessions) only.  Each
pool below -- 64 to 260 problems of one site -- is padded to one shape per family it can reach
(tests/helpers.py: pad_batch) and launched once per shape through the device entry with every output poisoned.  Then:
  * every output element is written, dead periods exactly zero;
  * every answer passes the certificate (SOLVED / SOLVED_INACCURATE / MAX_ITER limits, oracle/kkt.py);
  * the answers of one problem agree across its routes (schedules, repaired objective, status);
  * the union of the routes reached is all eleven families, and the polish solves problems on its routes.
Last, one acnqp_solve_batches call whose batches alternate padded shapes, with an empty batch, multiplier output on
some batches and a warm start on one, gives each batch the bits of its own solve()."""
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests.helpers import launch_poisoned as _launch_poisoned, route_shapes as _shapes

RATE_TOL = 1e-4 * 32.0   # north star: 1e-4 relative on rates, 32 A pilots (the hard limit across routes)
# |x_route - x_route'| of a problem SOLVED on both routes, per pool: 10x the worst difference measured on an MI355X (in
# brackets), capped by RATE_TOL.  The load-flattening pool sits at the solver's accuracy there: its rates are fixed
# only through pdiag = 2e-3 in the directions the flat row leaves free, so |q|_inf = 104 times eps 1e-8 becomes 5e-4 A
# (the certificate, which is what the answers owe, passes on every route).  Pairs with a SOLVED_INACCURATE answer are
# held to RATE_TOL.
ROUTE_RATE_TOL = {
    "ct54_soc": 2.1e-5,            # [2.02e-6]
    "ct54_soc_peak": 8.2e-5,       # [8.11e-6]
    "ct54_lin_peak_eq": 1.1e-7,    # [1.02e-8]
    "edges_n79_t17_soc": 7.5e-8,   # [7.44e-9]
    "edges_n60_t17_soc_peak": 0.0,  # (one route)
    "edges_jpl_t13_soc": 1.3e-4,   # [1.21e-5]
    "stalled": 1.1e-4,             # [1.06e-5]
    "edges_n100_t24_lf": RATE_TOL,  # [8.45e-4]
    "edges_jpl_t28_dc": 2e-10,     # [1.90e-11]
}
# repaired objective (obj + const) of a problem SOLVED on both routes: 1e-9 relative, except where the measured worst
# exceeds that -- 10x the measured worst there: the two pools whose rates differ most (jpl52, |x_a - x_b| 1.2e-5 A:
# 3.9e-9; load flattening: 9.3e-9).  Measured elsewhere: <= 7.9e-10.
ROUTE_OBJ_REL = {"edges_jpl_t13_soc": 3.9e-8, "edges_n100_t24_lf": 9.4e-8}
FAMILIES = {"wave1", "wave2", "wave3", "wave4", "wave5", "tiled_ct1", "tiled_ct2", "long_lds", "long_ws", "stream", "general"}


def _stalled_pool(copies=5):
    """the tests/golden/stalled.npz instances (configs[3] site 3, horizons 12 and 24), each as its own snapshot, ``copies``
    times over: problems that reach the polish hand-over"""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge
    from adacharge_amd.builder import ProblemBatch, build_batch, make_site

    g = H.load_stalled()
    names = [str(n) for n in g["names"]]
    parts, site = [], None
    for name in names:
        sl, infra, iface, meta, peak, exp = H.wide_case(g, name)
        if site is None:
            site = make_site(infra, meta["ct"])
        obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, meta["es"])]
        parts.append(build_batch([sl], infra, iface, obj, meta["ct"], meta["eq"], site=site))
    tm, k = max(p.Tm for p in parts), max(p.K for p in parts)
    one = ProblemBatch.concatenate([H.pad_batch(p, tm, k) for p in parts])
    return ProblemBatch.concatenate([one] * copies)


POOLS = {
    # caltech54 snapshots (one session per EVSE: the wave routes are reachable), horizons T, T - 2, T - 4 in each launch
    "ct54_soc": lambda: H.certificate_pool("caltech54", "SOC", 12, 64, 31, two=False),
    "ct54_soc_peak": lambda: H.certificate_pool("caltech54", "SOC", 12, 64, 32, two=False, peak="mixed"),
    "ct54_lin_peak_eq": lambda: H.certificate_pool("caltech54", "LINEAR", 12, 64, 34, eq=True, two=False, peak="mixed"),
    # edges.npz sites: wide (N = 79), 48 padded site rows (N = 60), two row tiles (jpl52)
    "edges_n79_t17_soc": lambda: H.edges_pool("n79_t17_soc", 64, 41),
    "edges_n60_t17_soc_peak": lambda: H.edges_pool("n60_t17_soc_peak", 64, 42),
    "edges_jpl_t13_soc": lambda: H.edges_pool("jpl_t13_soc", 64, 43),
    "stalled": _stalled_pool,
    "edges_n100_t24_lf": lambda: H.edges_pool("n100_t24_lf", 64, 44),
    "edges_jpl_t28_dc": lambda: H.edges_pool("jpl_t28_dc", 64, 45),
}


@functools.lru_cache(maxsize=None)
def _routed(name):
    """(pool, {family: (shape, padded batch, outputs)}, polish stats before/after) -- one launch per family"""
    from adacharge_amd.backend import SiteHandle

    pool = POOLS[name]()
    assert 64 <= pool.B <= 260, (name, pool.B)
    h = SiteHandle(pool.site, 0)
    before = h.polish_stats()
    runs = {}
    for fam, (t, k) in _shapes(h, pool).items():
        padded = H.pad_batch(pool, t, k)
        runs[fam] = ((t, k), padded, _launch_poisoned(h, padded), h.route(t, k, pool.B)[1])
    after = h.polish_stats()
    h.close()
    return pool, runs, before, after


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_every_route_writes_every_output_and_passes_the_certificate(name):
    pool, runs, _, _ = _routed(name)
    assert len(runs) >= 2 or name == "edges_n60_t17_soc_peak", (name, list(runs))
    for fam, ((t, k), padded, out, _) in runs.items():
        where = f"{name} on {fam} (t_max {t}, K {k})"
        for key in ("x", "y", "pri_res", "dua_res", "obj"):
            assert not np.isnan(out[key]).any(), f"{where}: {key} left unwritten"
        assert (out["iters"] >= 0).all(), f"{where}: iters left unwritten"
        assert np.isin(out["status"], (1, 2, 5)).all(), (where, out["status"])
        assert (out["status"] == 1).mean() >= 0.9, (where, np.bincount(out["status"]))
        for b in range(pool.B):
            T = int(pool.T[b])
            assert not out["x"][b][:, T:].any() and not out["y"][b][:, T:].any(), f"{where}: problem {b} dead periods"
            obj = out["obj"][b] + kkt.prox_terms(padded, b, out["x"][b])
            bad = kkt.failures(kkt.certify(padded, b, out["x"][b], out["y"][b], obj), int(out["status"][b]))
            assert not bad, f"{where}: problem {b} (T {T}, status {int(out['status'][b])}, iters {int(out['iters'][b])}): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_same_problem_same_answer_whatever_the_route(name):
    pool, runs, _, _ = _routed(name)
    fams = sorted(runs)
    ref = fams[0]
    worst = 0.0
    for fam in fams[1:]:
        a, b_ = runs[ref][2], runs[fam][2]
        for b in range(pool.B):
            T = int(pool.T[b])
            sa, sb = int(a["status"][b]), int(b_["status"][b])
            d = float(np.abs(a["x"][b][:, :T] - b_["x"][b][:, :T]).max())
            if sa == sb == 1:
                worst = max(worst, d)
                assert d <= ROUTE_RATE_TOL[name], (name, ref, fam, b, d)
                oa = a["obj"][b] + kkt.prox_terms(runs[ref][1], b, a["x"][b]) + pool.const[b]
                ob = b_["obj"][b] + kkt.prox_terms(runs[fam][1], b, b_["x"][b]) + pool.const[b]
                assert abs(oa - ob) <= ROUTE_OBJ_REL.get(name, 1e-9) * max(abs(oa), abs(ob)), (name, ref, fam, b, oa, ob)
            else:
                # a route without the polish may leave a stalled problem SOLVED_INACCURATE where a polishing one solves it
                assert {sa, sb} == {1, 5} or sa == sb == 5, (name, ref, fam, b, sa, sb)
                assert d <= RATE_TOL, (name, ref, fam, b, sa, sb, d)
    print(f"[route] {name}: {len(fams)} routes, worst SOLVED rate difference {worst:.3e} A")


@pytest.mark.gpu
def test_routes_cover_every_family_and_the_polish_solves():
    reached = set()
    for name in POOLS:
        reached |= set(_routed(name)[1])
    assert reached == FAMILIES, sorted(FAMILIES - reached)
    pool, runs, before, after = _routed("stalled")
    assert any(pol for (_, _, _, pol) in runs.values())
    assert after["solved"] > before["solved"], (before, after)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [True, False])
def test_mixed_shape_pipelined_call_gives_each_batch_its_own_bits(pinned):
    _mixed_shape_call(pinned, None)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [True, False])
def test_mixed_shape_pipelined_call_in_chunks_of_eight_gives_each_batch_its_own_bits(pinned, monkeypatch):
    """... with ACNQP_CHUNK=8 (read at every call) for the pipelined call only: the batches differ in shape and in
    want_y / warm start, so the call is not planned as a whole, and chunks also split inside a batch."""
    _mixed_shape_call(pinned, monkeypatch)


def _mixed_shape_call(pinned, chunked):
    """acnqp_solve_batches over batches that alternate padded shapes (so chunks split on the shape), with an empty batch,
    multiplier output on some and a warm start on one (chunks split on those too): each batch's bits equal its own
    solve() (the size-invariance rule, tests/test_batch_invariance.py)."""
    from adacharge_amd.backend import SiteHandle

    pool = POOLS["ct54_soc"]()
    h = SiteHandle(pool.site, 0)
    shapes = list(_shapes(h, pool).values())[:4]
    part = lambda lo, hi, s: H.pad_batch(pool.subset(np.arange(lo, hi)), *s)
    batches = [part(0, 16, shapes[0]), part(16, 16, shapes[1]), part(16, 32, shapes[1]), part(32, 40, shapes[0]),
               part(40, 52, shapes[2 % len(shapes)]), part(52, 64, shapes[3 % len(shapes)]), part(0, 16, shapes[0])]
    want_y = [True, False, False, True, True, False, True]
    first = h.solve(batches[0], want_y=True)
    warm = [None] * 6 + [(first.x, first.y)]
    if chunked is not None:
        chunked.setenv("ACNQP_CHUNK", "8")
    many = h.solve_many(batches, pinned_results=pinned, want_y=want_y, warm=warm)
    if chunked is not None:
        chunked.delenv("ACNQP_CHUNK")
    assert many[1].x.shape[0] == 0
    for g, (batch, res) in enumerate(zip(batches, many)):
        if batch.B == 0:
            continue
        own = h.solve(batch, want_y=want_y[g], warm=warm[g])
        for key in ("x", "status", "iters", "pri_res", "dua_res", "obj"):
            assert np.array_equal(getattr(own, key), getattr(res, key)), (g, batch.Tm, batch.K, key)
        if want_y[g]:
            assert np.array_equal(own.y, res.y), (g, "y")
        else:
            assert res.y is None
    h.close()
