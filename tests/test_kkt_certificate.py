"""The KKT certificate of one answer (oracle/kkt.py), on the CPU.

The C twin of the device algorithm (oracle/admm_port.c) at default options passes it on small pools of every
constraint family; each of a set of subtle corruptions of a passing answer -- a few milliamperes moved inside a
session, a multiplier off by 0.1 %, a rotated cone multiplier, a sign, a bit of a padded period, the objective's ninth
digit -- fails it; and padding a problem to another shape (tests/helpers.py: pad_batch) changes neither its statement
nor its certificate.  tests/test_route_certificate.py certifies every kernel route's answers with the same constants."""
import functools

import numpy as np
import pytest

from oracle import kkt
from tests import helpers as H

# name: pool generator (tests/helpers.py).  Snapshot pools mix horizons T, T - 2, T - 4 in one batch.
POOLS = {
    "ct54_soc_t12_eq_mixedpeak": lambda: H.certificate_pool("caltech54", "SOC", 12, 12, 11, eq=True, peak="mixed"),
    "ct54_lin_t12_vpeak": lambda: H.certificate_pool("caltech54", "LINEAR", 12, 12, 12, peak="vector"),
    "ct54_soc_t16_speak": lambda: H.certificate_pool("caltech54", "SOC", 16, 12, 13, peak="scalar"),
    "ct54_lin_t16_eq": lambda: H.certificate_pool("caltech54", "LINEAR", 16, 12, 14, eq=True),
    # the load-flattening and demand-charge cases of edges.npz that the twin solves quickly (test_golden_edges.SLOW_ON_CPU)
    "edges_n100_t24_lf": lambda: H.edges_pool("n100_t24_lf", 3, 1),
    "edges_jpl_t28_dc": lambda: H.edges_pool("jpl_t28_dc", 3, 2),
}


@functools.lru_cache(maxsize=None)
def _solved(name):
    """(batch, twin answers with the objective as SiteHandle reports it)"""
    from oracle import admm_port

    batch = POOLS[name]()
    out = admm_port.solve_batch(batch, threads=min(8, admm_port.max_threads()), accel_mem=5)
    out["obj"] = out["obj"] + np.array([kkt.prox_terms(batch, b, out["x"][b]) for b in range(batch.B)])
    return batch, out


def _cert(batch, out, b, x=None, y=None, obj=None):
    return kkt.certify(batch, b, out["x"][b] if x is None else x, out["y"][b] if y is None else y,
                       out["obj"][b] if obj is None else obj)


def test_pools_cover_the_families():
    shapes = {n: _solved(n)[0] for n in POOLS}
    assert {b.site.cone for b in shapes.values()} == {0, 1}
    assert all(b.K == 2 for n, b in shapes.items() if n.startswith("ct54"))
    assert all(len(set(b.T.tolist())) >= 3 for n, b in shapes.items() if n.startswith("ct54"))
    assert any(b.s_eq.all() for b in shapes.values())
    pk = shapes["ct54_soc_t12_eq_mixedpeak"].peak
    assert np.isinf(pk).all(axis=1).any() and np.isfinite(pk).all(axis=1).any()
    assert shapes["edges_n100_t24_lf"].site.has_flat and shapes["edges_jpl_t28_dc"].site.has_max


@pytest.mark.parametrize("name", list(POOLS))
def test_twin_answers_pass_the_certificate(name):
    batch, out = _solved(name)
    assert (out["status"] == kkt.ST_SOLVED).all(), (name, out["status"])
    for b in range(batch.B):
        bad = kkt.failures(_cert(batch, out, b), int(out["status"][b]))
        assert not bad, (name, b, bad)


# ---- the checker catches subtle errors ------------------------------------------------------------------------------
def _fails(batch, out, b, **kw):
    assert not kkt.failures(_cert(batch, out, b), kkt.ST_SOLVED)   # the unmutated answer passes
    return kkt.failures(_cert(batch, out, b, **kw), kkt.ST_SOLVED)


def test_rejects_rate_moved_between_free_periods_of_a_session():
    d = 3.2e-3   # the north-star rate tolerance
    batch, out = _solved("ct54_soc_t12_eq_mixedpeak")
    for b in range(batch.B):
        x = out["x"][b]
        for k in range(batch.K):
            for i in range(batch.N):
                L, o = int(batch.s_len[b, k, i]), int(batch.s_off[b, k, i])
                w = slice(o, o + L)
                free = np.flatnonzero((x[i, w] > batch.lb[b, i, w] + d) & (x[i, w] < batch.ub[b, i, w] - d)) + o
                if len(free) >= 2:
                    xm = x.copy()
                    xm[i, free[0]] += d
                    xm[i, free[1]] -= d
                    obj = 0.5 * batch.pdiag[b] * (xm * xm).sum() + (batch.q[b] * xm).sum()
                    bad = _fails(batch, out, b, x=xm, obj=obj)
                    assert "stat" in bad, bad
                    assert kkt.certify(batch, b, xm, out["y"][b], out["obj"][b])["energy"] <= kkt.EXACT_REL
                    return
    pytest.fail("no session with two free periods in the pool")


def test_rejects_largest_site_row_multiplier_scaled_by_1_001():
    for name in ("ct54_lin_t12_vpeak", "ct54_soc_t16_speak"):
        batch, out = _solved(name)
        b = int(np.argmax([np.abs(out["y"][k]).max() for k in range(batch.B)]))
        y = out["y"][b].copy()
        j, t = np.unravel_index(np.argmax(np.abs(y)), y.shape)
        y[j, t] *= 1.001
        assert _fails(batch, out, b, y=y), name


def test_rejects_multiplier_on_a_slack_row():
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
            bad = _fails(batch, out, b, y=ym)
            assert "comp" in bad, bad
            return
    pytest.fail("no slack row")


def test_rejects_rotated_cone_multiplier():
    batch, out = _solved("ct54_soc_t16_speak")
    M = batch.site.M
    lam = np.stack([np.hypot(out["y"][b][:M], out["y"][b][M:2 * M]) for b in range(batch.B)])
    b, j, t = np.unravel_index(np.argmax(lam), lam.shape)   # the most binding pair of the pool
    y = out["y"][b].copy()
    c, s = np.cos(1e-3), np.sin(1e-3)
    y[j, t], y[j + M, t] = c * y[j, t] - s * y[j + M, t], s * y[j, t] + c * y[j + M, t]
    bad = _fails(batch, out, b, y=y)
    assert "cone" in bad, bad


def test_rejects_max_row_multiplier_with_flipped_sign():
    batch, out = _solved("edges_jpl_t28_dc")
    r = batch.site.max_row
    y = out["y"][0].copy()
    t = int(np.argmax(y[r]))
    assert y[r, t] > 0
    y[r, t] = -y[r, t]
    bad = _fails(batch, out, 0, y=y)
    assert "dual" in bad, bad


def test_rejects_a_tiny_rate_in_a_padded_period():
    batch, out = _solved("ct54_soc_t12_eq_mixedpeak")
    b = int(np.flatnonzero(batch.T < batch.Tm)[0])
    x = out["x"][b].copy()
    x[0, batch.Tm - 1] = 1e-300
    bad = _fails(batch, out, b, x=x)
    assert "zero" in bad, bad


def test_rejects_objective_off_by_1e_9():
    for name in ("ct54_lin_t16_eq", "edges_n100_t24_lf", "edges_jpl_t28_dc"):
        batch, out = _solved(name)
        bad = _fails(batch, out, 0, obj=out["obj"][0] * (1 + 1e-9))
        assert "obj" in bad, (name, bad)


# ---- padding is inert -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ct54_soc_t12_eq_mixedpeak", "ct54_lin_t12_vpeak", "edges_n100_t24_lf", "edges_jpl_t28_dc"])
def test_padding_leaves_the_certificate_unchanged(name):
    batch, out = _solved(name)
    tm, k = batch.Tm + 7, batch.K + 3
    padded = H.pad_batch(batch, tm, k)
    xp, yp = H.pad_result(out["x"], tm), H.pad_result(out["y"], tm)
    for b in range(batch.B):
        a = _cert(batch, out, b)
        p = kkt.certify(padded, b, xp[b], yp[b], out["obj"][b])
        assert a.keys() == p.keys()
        for key in a:
            assert p[key] == pytest.approx(a[key], rel=1e-9, abs=1e-15), (name, b, key, a[key], p[key])


def test_pad_batch_matches_the_builders_statement():
    """A snapshot built alone and padded equals the same snapshot built inside a batch of a longer horizon and more
    session slots: the builder's dead periods and empty slots are exactly pad_batch's."""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
    rng = np.random.default_rng(7)
    short = sites.random_sessions(infra, 9, rng)
    long2 = sites.random_sessions_general(infra, 20, rng, two_per_evse=True)
    for ct, peaks in (("SOC", [400.0, None]), ("LINEAR", [rng.uniform(250, 600, size=9), 500.0])):
        both = build_batch([short, long2], infra, iface, obj, ct, peak_limits=peaks)
        alone = build_batch([short], infra, iface, obj, ct, peak_limits=peaks[:1])
        assert both.Tm == 20 and both.K == 2 and alone.Tm == 9 and alone.K == 1
        padded = H.pad_batch(alone, both.Tm, both.K)
        first = both.subset(np.arange(1))
        for key in ("T", "lb", "ub", "q", "pdiag", "lf", "s_off", "s_len", "s_cap", "s_eq", "peak", "dc", "dfloor", "const"):
            a, p = getattr(first, key), getattr(padded, key)
            assert (a is None) == (p is None), key
            if a is not None:
                assert a.shape == p.shape and np.array_equal(a, p), (ct, key)
