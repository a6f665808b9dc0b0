"""The verdicts other than SOLVED -- PRIMAL_INFEASIBLE (3), EMPTY_SET (4), MAX_ITER (2) -- of every kernel route, on the
problems of tests/verdict_cases.py: feasibility known without a solver tolerance, probes at relative offsets
d = +-{1e-2, 1e-3, 1e-4, 1e-5} from the boundary (tests/test_verdict_cases.py proves the truth and runs the CPU twins).

Each pool mixes the probes of one (site, cone) with ordinary problems that solve, is padded to the smallest shape of
each kernel family it reaches (tests/helpers.py: pad_batch, route_shapes) and launched once per family through the device
entry with every output poisoned.  Then, per route:
  1. no false alarm: a feasible probe ends 1 or 5 and passes oracle/kkt.py;
  2. no false answer: an infeasible probe never ends SOLVED at d >= 1e-4 (a SOLVED answer violates a site row by at most
     1.5e-6 max(1, limit)) and never SOLVED_INACCURATE at d = 1e-2 (1.5e-3); an answer passes kkt;
  3. the verdict of oracle/admm_port on every problem, the certificate in fewer than 5,000 iterations;
  4. the output contract of the unsolved (include/acn_qp.h);
  5. MAX_ITER with max_iter = check_every on every route;
  6. statuses 3, 4 and 2 are batch-size and position invariant, and leave their solved neighbours' bits alone;
  7. the dual report gives unsolved problems zeros and +inf, on both forms of its kernel;
  8. the Python surface raises / reports as the reference does."""
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H
from tests import verdict_cases as V

FAMILIES = {"wave1", "wave2", "wave3", "wave4", "wave5", "tiled_ct1", "tiled_ct2", "long_lds", "long_ws", "stream", "general"}
BIG = 1e300   # what every kernel writes to pri_res / dua_res of an EMPTY_SET problem
POOL_SIZE = 48

# name -> site, cone, peak row, session slots, kernel families to launch (None: every family the pool reaches).  The
# padded horizon 289 (GENERAL on a site of one or two row tiles) is left to the narrow sites.
POOLS = {
    "n8_soc": dict(site="n8", cone="SOC", peak=False, k=1, want=None),
    "n8_lin_peak": dict(site="n8", cone="LINEAR", peak=True, k=1, want=FAMILIES - {"general"}),
    "pods18_lin": dict(site="pods18", cone="LINEAR", peak=False, k=1, want=FAMILIES - {"general"}),
    "pods18_lin_peak": dict(site="pods18", cone="LINEAR", peak=True, k=1, want={"wave3", "wave4", "long_lds"}),
    "pods18_soc_peak": dict(site="pods18", cone="SOC", peak=True, k=1, want={"general"}),
    "wide80_soc": dict(site="wide80", cone="SOC", peak=False, k=1, want={"stream"}),
    "wide80_lin_peak": dict(site="wide80", cone="LINEAR", peak=True, k=1, want={"stream"}),
    "n2_t40_lin": dict(site="n2_t40", cone="LINEAR", peak=False, k=1, want={"wave5", "long_ws"}),
    "n2_t96_soc": dict(site="n2_t96", cone="SOC", peak=False, k=1, want={"long_ws"}),
    "n2_t144_lin": dict(site="n2_t144", cone="LINEAR", peak=False, k=1, want={"long_ws"}),
    # family (d): sites.caltech54(), three phases, eight rows (one row tile in both cones)
    "ct54_lin": dict(site="caltech54", cone="LINEAR", peak=False, k=1, want=FAMILIES - {"general"}),
    "ct54_soc": dict(site="caltech54", cone="SOC", peak=False, k=1, want=FAMILIES - {"general"}),
    # the remaining (site, cone, peak) combinations of the grid, so that every generated probe meets a kernel
    "n2_lin": dict(site="n2", cone="LINEAR", peak=False, k=1, want=FAMILIES - {"general"}),
    "n2_soc": dict(site="n2", cone="SOC", peak=False, k=1, want=FAMILIES - {"general"}),
    "n30_lin": dict(site="n30", cone="LINEAR", peak=False, k=1, want=FAMILIES - {"general"}),
    "n30_soc": dict(site="n30", cone="SOC", peak=False, k=1, want=FAMILIES - {"general"}),
    "n8_lin": dict(site="n8", cone="LINEAR", peak=False, k=1, want=FAMILIES - {"general"}),
    "n8_soc_peak": dict(site="n8", cone="SOC", peak=True, k=1, want=FAMILIES - {"general"}),
    "pods18_soc": dict(site="pods18", cone="SOC", peak=False, k=1, want={"general"}),
    "wide80_lin": dict(site="wide80", cone="LINEAR", peak=False, k=1, want={"stream"}),
    "wide80_soc_peak": dict(site="wide80", cone="SOC", peak=True, k=1, want={"stream"}),
    "n2_t40_soc": dict(site="n2_t40", cone="SOC", peak=False, k=1, want={"wave5", "long_ws"}),
    "n2_t96_lin": dict(site="n2_t96", cone="LINEAR", peak=False, k=1, want={"long_ws"}),
    "n2_t144_soc": dict(site="n2_t144", cone="SOC", peak=False, k=1, want={"long_ws"}),
    "e_k2": dict(site="n8", cone="SOC", peak=False, k=2, want=FAMILIES - {"general"}),
    "e_k4": dict(site="n8", cone="SOC", peak=False, k=4, want=FAMILIES - {"general"}),
}
MAX_ITER_POOLS = ("n8_soc", "pods18_lin", "wide80_soc", "n2_t96_soc")


@functools.lru_cache(maxsize=None)
def _all_cases():
    return [c for f in V.FAMILIES for c in V.FAMILIES[f]()]


def _filler(spec, rng, n):
    if spec["site"] == "caltech54":
        return [V.site_scaling(int(rng.integers(0, len(V.D_SEEDS))), spec["cone"], -float(rng.uniform(0.1, 0.5))).batch for _ in range(n)]
    if spec["peak"]:
        return [V.peak_cause(spec["site"], spec["cone"], -float(rng.uniform(0.1, 0.6)), "eq").batch for _ in range(n)]
    return V.solved_filler(spec["site"], spec["cone"], rng, n)


@functools.lru_cache(maxsize=None)
def _pool(name):
    """(probes, batch): the probes of the pool's (site, cone, peak, slots) first, then ordinary problems that solve"""
    from adacharge_amd.builder import ProblemBatch

    spec = POOLS[name]
    probes = [c for c in _all_cases() if (c.site, c.cone) == (spec["site"], spec["cone"])
              and (c.batch.peak is not None) == spec["peak"] and c.batch.K == spec["k"]]
    assert len(probes) >= 8, name
    rng = np.random.default_rng(sum(map(ord, name)))
    fill = _filler(spec, rng, max(POOL_SIZE - len(probes), 16))
    parts = [c.batch for c in probes] + fill
    tm, k = max(p.Tm for p in parts), max(p.K for p in parts)
    return probes, ProblemBatch.concatenate([H.pad_batch(p, tm, k) for p in parts])


@functools.lru_cache(maxsize=None)
def _routed(name):
    """{family: (shape, padded batch, outputs, twin outputs)} -- one poisoned launch per family of the pool"""
    from adacharge_amd.backend import SiteHandle, default_options
    from oracle import admm_port

    probes, pool = _pool(name)
    h = SiteHandle(pool.site, 0)
    runs = {}
    for fam, (t, k) in H.route_shapes(h, pool).items():
        if POOLS[name]["want"] is not None and fam not in POOLS[name]["want"]:
            continue
        padded = H.pad_batch(pool, t, k)
        assert h.route(t, k, padded.B)[0] == fam
        out = H.launch_poisoned(h, padded)
        twin = admm_port.solve_batch(padded, threads=16, accel_mem=h.accel_columns(t, k, default_options()))
        runs[fam] = ((t, k), padded, out, twin)
    h.close()
    assert runs, name
    return runs


def _certified(padded, b, out):
    obj = out["obj"][b] + kkt.prox_terms(padded, b, out["x"][b])
    return kkt.failures(kkt.certify(padded, b, out["x"][b], out["y"][b], obj), int(out["status"][b]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_no_false_alarm_no_false_answer_and_the_twins_verdict(name):
    probes, pool = _pool(name)
    for fam, ((t, k), padded, out, twin) in _routed(name).items():
        where = f"{name} on {fam} (t_max {t}, K {k})"
        st, it = out["status"], out["iters"]
        print(f"[verdict] {where}: statuses {np.bincount(st, minlength=6).tolist()}, certificate iterations "
              f"{sorted(set(it[st == 3].tolist()))}")
        for b, c in enumerate(probes):
            s = int(st[b])
            tag = f"{where}: {c.name} status {s} iters {int(it[b])}"
            if c.truth == "feasible":   # 1. no false alarm
                assert s in (1, 5), tag
            else:                       # 2. no false answer
                assert not (s == 1 and c.d >= 1e-4), tag
                assert not (s in (1, 5) and c.d >= 1e-2), tag
            if s in (1, 5):
                bad = _certified(padded, b, out)
                assert not bad, (tag, bad)
            assert s == c.expected, tag   # 3. what the twin gives (tests/test_verdict_cases.py: the truth, on every probe)
        assert np.array_equal(st, twin["status"]), (where, np.flatnonzero(st != twin["status"]), st, twin["status"])
        assert (it[st == 3] < 5000).all(), (where, it[st == 3])
        for b in range(len(probes), pool.B):   # the ordinary neighbours solve, certified
            assert int(st[b]) == 1, (where, b, int(st[b]))
            assert not _certified(padded, b, out), (where, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_output_contract_of_the_unsolved(name):
    """include/acn_qp.h, next to acnqp_results: what x, y, obj, pri_res, dua_res and iters hold for statuses 3 and 4"""
    probes, pool = _pool(name)
    for fam, ((t, k), padded, out, _) in _routed(name).items():
        where = f"{name} on {fam} (t_max {t}, K {k})"
        for key in ("x", "y", "pri_res", "dua_res", "obj"):
            assert not np.isnan(out[key]).any(), f"{where}: {key} left unwritten"
        assert (out["iters"] >= 0).all() and (out["status"] != 0).all(), f"{where}: iters / status left unwritten"
        for b in np.flatnonzero(out["status"] == 3):
            # the feasible ADMM iterate: inside the box, exact zeros outside the windows and at dead periods, all finite
            cert = kkt.certify(padded, b, out["x"][b], out["y"][b], out["obj"][b])
            assert not kkt.failures(cert, 3), (where, b, kkt.failures(cert, 3))
            # ... and on the energy rows: the projection stops at 6.4e-12 max(1, |cap|) (64 x proj_tol); 1e-9 is far above
            # that and far below any residual tolerance
            assert cert["energy"] <= 1e-9, (where, b, cert["energy"])
            assert cert["obj"] <= kkt.EXACT_REL, (where, b, cert["obj"])
            assert np.isfinite(out["pri_res"][b]) and np.isfinite(out["dua_res"][b]) and out["iters"][b] > 0
            assert not out["y"][b][:, int(padded.T[b]):].any(), (where, b)
        for b in np.flatnonzero(out["status"] == 4):
            assert not out["x"][b].any() and not out["y"][b].any(), (where, b)
            assert out["iters"][b] == 0 and out["obj"][b] == 0.0, (where, b, out["iters"][b], out["obj"][b])
            assert out["pri_res"][b] == BIG and out["dua_res"][b] == BIG, (where, b, out["pri_res"][b], out["dua_res"][b])


@pytest.mark.gpu
def test_pools_cover_every_family_with_both_sides_of_the_boundary():
    reached = {f: set() for f in FAMILIES}
    for name in POOLS:
        probes, _ = _pool(name)
        for fam in _routed(name):
            reached[fam] |= {c.truth for c in probes}
    print("[verdict] families reached:", {f: sorted(v) for f, v in sorted(reached.items())})
    for fam in FAMILIES:
        assert {"feasible", "infeasible"} <= reached[fam], (fam, reached[fam])
        assert "empty_set" in reached[fam], (fam, reached[fam])


# ---- 5. MAX_ITER ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _max_iter_runs(name):
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import ProblemBatch
    from oracle import admm_port

    spec = POOLS[name]
    pool = ProblemBatch.concatenate(_filler(spec, np.random.default_rng(77), 24))
    h = SiteHandle(pool.site, 0)
    opts = default_options(max_iter=20, check_every=20)
    runs = {}
    for fam, (t, k) in H.route_shapes(h, pool).items():
        if name != "n8_soc" and fam not in ("wave3", "wave4", "long_lds", "stream", "long_ws"):
            continue
        padded = H.pad_batch(pool, t, k)
        twin = admm_port.solve_batch(padded, threads=16, max_iter=20, check_every=20, accel_mem=h.accel_columns(t, k, opts))
        runs[fam] = ((t, k), padded, H.launch_poisoned(h, padded, opts), twin)
    h.close()
    return runs


@pytest.mark.gpu
def test_max_iter_on_every_route():
    """max_iter = check_every = 20 on pools whose feeders bind: every problem ends MAX_ITER after exactly max_iter
    iterations (as in the twin), with every output written, finite and inside the box."""
    reached = set()
    for name in MAX_ITER_POOLS:
        for fam, ((t, k), padded, out, twin) in _max_iter_runs(name).items():
            where = f"{name} on {fam} (t_max {t}, K {k})"
            reached.add(fam)
            assert (twin["status"] == 2).all() and (twin["iters"] == 20).all(), (where, twin["status"], twin["iters"])
            assert (out["status"] == 2).all() and (out["iters"] == 20).all(), (where, out["status"], out["iters"])
            for key in ("x", "y", "pri_res", "dua_res", "obj"):
                assert np.isfinite(out[key]).all(), f"{where}: {key}"
            for b in range(padded.B):
                cert = kkt.certify(padded, b, out["x"][b], out["y"][b], out["obj"][b])
                assert not kkt.failures(cert, 2), (where, b, kkt.failures(cert, 2))
                assert cert["energy"] <= 1e-9 and cert["obj"] <= kkt.EXACT_REL, (where, b, cert["energy"], cert["obj"])
    assert reached == FAMILIES, sorted(FAMILIES - reached)


# ---- 6. invariance -----------------------------------------------------------------------------------------------------
INVARIANCE = {   # family -> (pool, padded shape)
    "wave1": ("n8_soc", (12, 1)), "wave4": ("pods18_lin", (13, 1)), "tiled_ct1": ("n8_soc", (12, 2)),
    "long_lds": ("pods18_lin", (17, 2)), "long_ws": ("n8_soc", (49, 1)), "stream": ("wide80_soc", (12, 1)),
    "general": ("n8_soc", (289, 1)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(INVARIANCE))
def test_unsolved_problems_are_batch_and_position_invariant(family):
    """A problem ending 3, one ending 4 and a second one ending 3 give the same bits of status, iters and x alone and at
    positions 0, 128 and 256 (each special at each position: three rotations) of a launch of 257 whose other 254
    problems solve; those 254 give the bits they give without them.  The same under max_iter = check_every = 20, where
    every problem but the empty one ends 2."""
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import ProblemBatch

    name, (t, k) = INVARIANCE[family]
    spec = POOLS[name]
    probes, _ = _pool(name)
    pick = lambda fam, d: next(c for c in probes if c.family == fam and c.d == d and (fam != "e" or "ub_eq" in c.name))
    specials = [H.pad_batch(pick(f, d).batch, t, k) for f, d in (("a", 1e-3), ("e", 1e-3), ("b", 1e-2))]
    distinct = ProblemBatch.concatenate([H.pad_batch(p, t, k) for p in _filler(spec, np.random.default_rng(5), 32)])
    fill = distinct.subset(np.arange(254) % 32)
    h = SiteHandle(fill.site, 0)
    assert h.route(t, k, 257)[0] == family and h.route(t, k, 1)[0] == family
    keys = ("status", "iters", "x")
    for opts, want in ((None, [3, 4, 3]), (default_options(max_iter=20, check_every=20), [2, 4, 2])):
        base = H.launch_poisoned(h, fill, opts)
        assert (base["status"] == (1 if opts is None else 2)).all(), (family, np.bincount(base["status"]))
        alone = [H.launch_poisoned(h, s, opts) for s in specials]
        assert [int(a["status"][0]) for a in alone] == want, (family, [int(a["status"][0]) for a in alone])
        for r in range(3):
            order = [specials[(j + r) % 3] for j in range(3)]
            mixed = ProblemBatch.concatenate([order[0], fill.subset(slice(0, 127)), order[1], fill.subset(slice(127, 254)), order[2]])
            assert mixed.B == 257
            out = H.launch_poisoned(h, mixed, opts)
            for j, pos in enumerate((0, 128, 256)):
                for key in keys:
                    assert np.array_equal(out[key][pos], alone[(j + r) % 3][key][0]), (family, r, pos, key)
            rest = np.r_[1:128, 129:256]
            for key in keys + ("y", "obj", "pri_res", "dua_res"):
                assert np.array_equal(out[key][rest], base[key]), (family, r, key)
    h.close()


# ---- 7. dual report ------------------------------------------------------------------------------------------------------
def _duals(h, dev):
    import torch

    mk = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
    mu, z, res = mk(dev.B, dev.K, dev.N), mk(dev.B, dev.N, dev.Tm), mk(dev.B, 4)
    h.duals_device(dev, mu, res, z=z, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return mu.cpu().numpy(), z.cpu().numpy(), res.cpu().numpy()


def _solved_dev(h, batch, options=None):
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = DeviceBatch(batch, "cuda:0", want_y=True)
    h.solve_device(dev, options, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name,one_wave", [("pods18_lin", True), ("wide80_soc", False)])
def test_dual_report_of_the_unsolved(name, one_wave):
    """acnqp_duals_device on a launch holding statuses 1, 3, 4 and 2 as the solver wrote them (the MAX_ITER ones by a
    solve with max_iter = check_every = 20): exact zeros in mu and z and four +inf for every unsolved problem; the solved
    ones bit-equal to a launch without the unsolved ones."""
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import ProblemBatch

    probes, pool = _pool(name)
    # the rule of acn_qp_duals.hpp (duals_wave_shape): the one-wavefront form serves N <= 64 with a padded horizon <= 16, the workgroup form
    # the rest -- the two pools sit on either side of it
    assert (pool.N <= 64 and pool.Tm <= 16) == one_wave, (name, pool.N, pool.Tm)
    n_cut = 6
    h = SiteHandle(pool.site, 0)
    dev = _solved_dev(h, pool)
    late = _solved_dev(h, pool.subset(slice(pool.B - n_cut, pool.B)), default_options(max_iter=20, check_every=20))
    for key in ("x", "y", "status"):
        getattr(dev, key)[pool.B - n_cut:] = getattr(late, key)
    st = dev.status.cpu().numpy()
    assert {1, 2, 3, 4} <= set(st.tolist()) and (st[-n_cut:] == 2).all(), np.bincount(st)
    mu, z, res = _duals(h, dev)
    unsolved = ~np.isin(st, (1, 5))
    assert not mu[unsolved].any() and not z[unsolved].any(), name
    assert np.isposinf(res[unsolved]).all(), (name, res[unsolved])
    assert np.isfinite(res[~unsolved]).all() and np.isfinite(mu[~unsolved]).all() and np.isfinite(z[~unsolved]).all()
    keep = np.flatnonzero(~unsolved)
    only = _solved_dev(h, pool.subset(keep))
    assert np.array_equal(only.status.cpu().numpy(), st[keep]) and np.array_equal(only.x.cpu().numpy(), dev.x.cpu().numpy()[keep])
    mu2, z2, res2 = _duals(h, only)
    assert np.array_equal(mu2, mu[keep]) and np.array_equal(z2, z[keep]) and np.array_equal(res2, res[keep]), name
    h.close()


# ---- 8. the Python surface ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_surface_raises_and_reports_as_the_reference_does():
    from adacharge_amd import AdaptiveChargingOptimization, InfeasibilityException

    infra, iface, obj, _ = V._context("n8", "SOC")
    ok, bad = V.feeder_equalities("n8", "SOC", -1e-3), V.feeder_equalities("n8", "SOC", 1e-3)
    # a session owed 33 A x 12 periods behind a 32 A pilot: its own bounds miss its energy equality
    empty = list(ok.sessions[1:]) + [V._session(infra, 0, 33.0 * 12, 0, 12)]
    opt = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", enforce_energy_equality=True)
    rates = opt.solve(ok.sessions, infra)
    assert rates.shape == (8, 12) and int(opt.last_result.status[0]) in (1, 5)
    for sessions, status in ((bad.sessions, 3), (empty, 4)):
        with pytest.raises(InfeasibilityException, match="Solve failed with status infeasible"):
            opt.solve(sessions, infra)
        assert int(opt.last_result.status[0]) == status
    rates, status = opt.solve_batch([ok.sessions, bad.sessions, empty], infra)
    assert status.tolist() == [1, 3, 4] and len(rates) == 3
    assert opt.dual_values(ok.sessions, infra, b=0)
    for b, sessions in ((1, bad.sessions), (2, empty)):
        with pytest.raises(InfeasibilityException, match=f"problem {b} ended with status infeasible: no dual values"):
            opt.dual_values(sessions, infra, b=b)
