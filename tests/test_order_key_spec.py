"""tests/order_key_spec.py (the numpy definition of the launch-order key) on hand-made problems with known answers, and
the one property the key's design rests on: on the bench's problems `no overloaded cell` is exactly `the twin converges
at its first residual check`."""
from types import SimpleNamespace

import numpy as np

from tests import order_key_spec as spec

INF = np.inf


def problem(G, limits, cone, ub, windows, caps, lb=None, horizon=None, peak=None, has_peak=False):
    """ONE problem: ub (N, Tm); windows[k][i] = (off, len) and caps[k][i] per session slot k and EVSE i"""
    ub = np.asarray(ub, float)[None]
    lb = np.zeros_like(ub) if lb is None else np.asarray(lb, float)[None]
    G = np.asarray(G, float).reshape(-1, ub.shape[1])
    w = np.asarray(windows, np.int32)[None]   # (1, K, N, 2)
    site = SimpleNamespace(G=G, M=len(limits), limits=np.asarray(limits, float), cone=cone, has_peak=has_peak)
    return SimpleNamespace(site=site, lb=lb, ub=ub, s_off=w[..., 0], s_len=w[..., 1], s_cap=np.asarray(caps, float)[None],
                           T=np.array([ub.shape[2] if horizon is None else horizon], np.int32),
                           peak=None if peak is None else np.asarray(peak, float)[None])


def answer(p):
    x0 = spec.greedy_schedule(p.lb, p.ub, p.s_off, p.s_len, p.s_cap, p.T)
    _, C, key = spec.describe(p)
    return x0[0], int(C[0]), int(key[0])


def test_empty_site_gives_key_zero():
    # rows but no session; a session but no row
    assert answer(problem([[1, 1]], [10.0], 0, np.full((2, 3), 8.0), [[(0, 0), (0, 0)]], [[0.0, 0.0]]))[1:] == (0, 0)
    x0, C, key = answer(problem(np.zeros((0, 2)), [], 1, np.full((2, 3), 8.0), [[(0, 3), (0, 0)]], [[12.0, 0.0]]))
    assert np.array_equal(x0, [[8, 4, 0], [0, 0, 0]]) and (C, key) == (0, 0)


def test_one_disc_pair_overloaded_in_exactly_one_period():
    # rows (re, im) = (x_0, x_1), limit 5: neither EVSE alone exceeds it, hypot(3, 4.5) = 5.41 does
    x0, C, key = answer(problem([[1, 0], [0, 1]], [5.0], 1, [[3.0, 3.0], [4.5, 4.5]], [[(0, 2), (0, 2)]], [[3.0, 4.5]]))
    assert np.array_equal(x0, [[3, 0], [4.5, 0]]) and (C, key) == (1, 8)
    assert np.allclose(spec.cell_ratios(problem([[1, 0], [0, 1]], [5.0], 1, [[3.0, 3.0], [4.5, 4.5]], [[(0, 2), (0, 2)]], [[3.0, 4.5]]).site,
                                        x0[None])[0], [[np.hypot(3, 4.5) / 5, 0]])


def test_box_row():
    x0, C, key = answer(problem([[1, 1]], [10.0], 0, np.full((2, 3), 8.0), [[(0, 3), (0, 3)]], [[12.0, 12.0]]))
    assert np.array_equal(x0, [[8, 4, 0], [8, 4, 0]]) and (C, key) == (1, 8)   # loads 16, 8, 0 against 10


def test_peak_row_with_one_finite_limit():
    # the box row never binds; the peak row's load is 16, 8, 0: period 0 has no limit, period 1 has 7
    kw = dict(G=[[1, 1], [1, 1]], limits=[100.0], cone=0, ub=np.full((2, 3), 8.0), windows=[[(0, 3), (0, 3)]], caps=[[12.0, 12.0]], has_peak=True)
    assert answer(problem(peak=[INF, 7.0, INF], **kw))[1:] == (1, 8)
    assert answer(problem(peak=[INF, 9.0, INF], **kw))[1:] == (0, 0)
    assert answer(problem(peak=[INF, INF, INF], **kw))[1:] == (0, 0)


def test_two_session_slots_on_one_evse():
    x0, C, key = answer(problem([[1]], [5.0], 0, np.full((1, 5), 8.0), [[(0, 2)], [(3, 2)]], [[10.0], [20.0]]))
    assert np.array_equal(x0, [[8, 2, 0, 8, 8]]) and (C, key) == (3, 24)


def test_horizon_shorter_than_the_padded_one():
    x0, C, key = answer(problem([[1]], [5.0], 0, np.full((1, 4), 8.0), [[(0, 4)]], [[100.0]], horizon=2))
    assert np.array_equal(x0, [[8, 8, 0, 0]]) and (C, key) == (2, 16)


def test_minimum_rates():
    kw = dict(G=[[1]], limits=[5.0], cone=0, ub=np.full((1, 3), 8.0), windows=[[(0, 3)]], caps=[[10.0]])
    x0, C, key = answer(problem(lb=np.full((1, 3), 6.0), **kw))
    assert np.array_equal(x0, [[8, 6, 6]]) and (C, key) == (3, 24)   # the minimum rate is charged beyond the cap
    x0, C, key = answer(problem(**kw))
    assert np.array_equal(x0, [[8, 2, 0]]) and (C, key) == (1, 8)


def test_key_packs_cells_and_sessions_into_1024_buckets():
    C, n = np.array([0, 0, 1, 3, 127, 500]), np.array([7, 17, 8, 200, 63, 64])
    assert spec.key_of(C, n).tolist() == [0, 2, 9, 31, 1023, 1023] and spec.key_of(C, n).dtype == np.int32


def test_no_overloaded_cell_is_convergence_at_the_first_check():
    """1,024 problems of the bench's generator (rank 0, batches 0 ... 3): C == 0 <=> the twin reports 20 iterations"""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch, make_site
    from oracle import admm_port

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    objective = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    site = make_site(infra, "SOC")
    C, iters = [], []
    for g in range(4):
        batch = build_batch(sites.snapshot_batch(infra, 12, 256, seed=20240 + 104729 * g), infra, iface, objective, "SOC", site=site)
        C.append(spec.describe(batch)[1])
        iters.append(admm_port.solve_batch(batch, threads=min(8, admm_port.max_threads()), accel_mem=5)["iters"])
    C, iters = np.concatenate(C), np.concatenate(iters)
    assert C.size == 1024 and 0 < (C == 0).sum() < 1024
    assert np.array_equal(C == 0, iters == 20)
