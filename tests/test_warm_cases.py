"""The reference of tests/test_warm_gpu.py alone (CPU): the warm points of tests/warm_cases.py on oracle/admm_port.

  * padding the problem and the warm arrays changes none of the twin's bits, so its answer at a pool's own shape stands for
    every padded shape the GPU test launches;
  * every kind of warm point is told apart from the cold start and from every other kind, on at least half of a pool, by
    what the GPU test asserts -- a warm start a kernel took wrongly (or not at all) could otherwise pass;
  * from ``exact`` the twin is done at the first check, and its own move from (x*, y*) is recorded;
  * oracle/admm_ref (readable numpy, written from the sentence in include/acn_qp.h) grounds the twin's warm start;
  * warm_y entries at dead periods are read as zero: y stays exactly zero there and no live output moves."""
import itertools

import numpy as np
import pytest

from tests import helpers as H
from tests import options_cases as OC
from tests import warm_cases as WC

MIN_SHARE = 0.5
# (pool, kind): share told apart in its worst pairing -- left out after measuring, one kind of a pool at the most.
# n100_t24_lf: the load-flattening cost has q = 0 up to the equal-share term, so the cold start -1e5 q projects to the point
# zero projects to (1.3e-9 A apart after one iteration; 17 A apart after sixty, where y2 = 0 against none differs)
LEFT_OUT = {("n100_t24_lf", "zero"): 0.0}
OUTPUTS = ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")


def _same_bits(a, b, t_max, where):
    for key in OUTPUTS:
        pa = H.pad_result(a[key], t_max) if key in ("x", "y") else a[key]
        assert np.array_equal(pa, b[key]), (where, key)


@pytest.mark.parametrize("name,shape", [("n8_soc", (13, 2)), ("n8_soc", (49, 1)), ("pods18_lin", (25, 1)), ("ct54_soc_mixed", (13, 1)),
                                        ("ct54_lin_eq_mixed", (25, 5)), ("n100_t24_lf", (49, 1)), ("jpl_t28_dc", (28, 2))])
def test_padding_leaves_the_warm_twin_alone(name, shape):
    """dead periods and empty slots added to the problem, and to the warm arrays zeros (``exact``, ``zero``, ``shifted``),
    U(-5, 40) in warm_x (``perturbed``: the projection removes it) or U(-3, 3) in warm_y (``stale``: read as zero)"""
    for kind in WC.kinds_of(name, shape[0]):
        for run in ("one", "m60", "full"):
            _same_bits(WC.twin(name, kind, run), WC.twin(name, kind, run, *shape), shape[0], (name, shape, kind, run))
    x0, y0 = WC.warm(name, "perturbed", shape[0])
    own = WC.pool(name).Tm
    assert (np.abs(x0[..., own:]) > 0).all() and not y0[..., own:].any()
    assert all(np.array_equal(a[..., :own], b) for a, b in zip((x0, y0), WC.warm(name, "perturbed")))


def test_padded_periods_move_the_max_row_by_roundoff_only():
    """the demand-charge prox couples all t_max periods (Newton on tau from max_t zh_t - dc / rho: while tau < 0 the dead
    periods, zh = 0, are in its sums), so dead periods added to jpl_t28_dc change the twin's last bits, cold or warm: sixty
    iterations of sums of values up to 40 A, 1e-11 A at the most -- tests/test_warm_gpu.py takes the twin at the padded shape"""
    name = "jpl_t28_dc"
    for kind in ("cold",) + WC.kinds_of(name, 33):
        for run in ("one", "m60"):
            a, b = WC.twin(name, kind, run), WC.twin(name, kind, run, 33)
            assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"]), (kind, run)
            dx, dy = (float(np.abs(H.pad_result(a[key], 33) - b[key]).max()) for key in ("x", "y"))
            print(f"[warm] {name} padded to 33 periods, {kind} {run}: |x - x_own| {dx:.2e} A, |y - y_own| {dy:.2e}")
            assert dx <= 1e-11 and dy <= 1e-11 and not b["y"][..., 28:].any() and not b["x"][..., 28:].any(), (kind, run, dx, dy)
            assert WC.twin_padded(name, kind, run, 33) is not a and np.array_equal(WC.twin_padded(name, kind, run, 33)["x"], b["x"])


@pytest.mark.parametrize("name", list(WC.POOLS))
def test_every_kind_is_told_apart(name):
    """At each limit of layer A every kind differs from the cold start and from every other kind by more than ten TRAJ_TOL
    in |x|_inf on at least half of the pool (``stale`` is ``exact`` at live periods: exempt).  Also the cap on the trajectory
    tolerances: a tenth of the smallest told-apart distance (the median of a pairing: half of the pool is at least as far)."""
    batch = WC.pool(name)
    worst, smallest = {}, np.inf
    for run in WC.LAYER_A:
        for a, b in itertools.combinations(("cold",) + WC.KINDS, 2):
            d = np.abs(WC.twin(name, a, run)["x"] - WC.twin(name, b, run)["x"]).reshape(batch.B, -1).max(axis=1)
            share = float((d > 10.0 * OC.TRAJ_TOL).mean())
            print(f"[warm] {name:18s} {run:4s} {a:9s} against {b:9s}: told apart {share:.2f}, median |x_a - x_b| {np.median(d):.2e} A, smallest {d.min():.2e} A")
            worst[b] = min(worst.get(b, 1.0), share)
            if share >= MIN_SHARE:
                smallest = min(smallest, float(np.median(d)))
    missed = {(name, k): s for k, s in worst.items() if s < MIN_SHARE}
    for (_, k), s in missed.items():
        print(f"[warm] {name}: {k} LEFT OUT (told apart {s:.2f} in its worst pairing)")
    assert len(missed) <= 1, missed
    assert set(missed) == {key for key in LEFT_OUT if key[0] == name}, missed
    for key, s in missed.items():
        assert abs(LEFT_OUT[key] - s) <= 0.0051, (key, s)
    print(f"[warm] {name}: smallest told-apart distance {smallest:.2e} A, TRAJ_TOL {OC.TRAJ_TOL:.1e} A")
    assert OC.TRAJ_TOL <= smallest / 10.0, (name, smallest)


def test_status_at_a_limit_does_not_hang_on_the_threshold():
    """no problem of a truncated run ends on the line between MAX_ITER and SOLVED_INACCURATE: the GPU test holds every status"""
    for name in WC.POOLS:
        for kind in WC.kinds_of(name, 10 ** 6):
            for run in WC.STALE_RUNS:
                assert WC.fragile(name, kind, run) == (), (name, kind, run)


def test_exact_is_done_at_the_first_check():
    """from (x*, y*) at eps = 1e-10 the twin ends SOLVED at iters == check_every under default options (no Anderson columns);
    its own move |x - x*|_inf is what tests/test_warm_gpu.py allows a kernel ten times of"""
    for name in WC.POOLS:
        out = WC.twin(name, "exact", "plain")
        assert (out["status"] == 1).all() and (out["iters"] == WC.check_period("plain")).all(), (name, out["status"], out["iters"])
        move = float(np.abs(out["x"] - WC.cold_answer(name)["x"]).max())
        print(f"[warm] {name}: the twin's own move from exact {move:.2e} A (recorded {WC.EXACT_MOVE[name]:.2e} A)")
        assert move <= WC.EXACT_MOVE[name] <= max(1.25 * move, move + 1e-9), (name, move)
        assert 10.0 * WC.EXACT_MOVE[name] <= OC.RATE_TOL, name


@pytest.mark.parametrize("name,t_max", [("n8_soc", 13), ("n2_t40_lin", 49)])
def test_numpy_restatement_grounds_the_warm_twin(name, t_max):
    """oracle/admm_ref takes warm_x / warm_y as include/acn_qp.h states them (z = Proj(warm_x), y2 = warm_y, y1 = -(P z +
    q + G' y2)); the twin follows it from every kind, one period of padding included (``stale`` has entries to ignore there).
    Full solves as tests/test_options_cases.py::test_numpy_restatement_grounds_the_twin_under_the_options: both solve, counts
    within 20, schedules within 1e-6 A.  One iteration from the start point -- the same sums in another order, values up to
    40 A and multipliers of order 1 -- to 1e-9 A, and y to 1e-9 of max(1, |y|_inf)."""
    from oracle.admm_ref import AdmmOptions, solve_one

    batch = H.pad_batch(WC.pool(name), t_max, WC.pool(name).K)
    for kind in WC.kinds_of(name, t_max):
        x0, y0 = WC.warm(name, kind, t_max)
        port1, port = WC.twin(name, kind, "one", t_max), WC.twin(name, kind, "full", t_max)
        for b in (0, 1):
            one = solve_one(batch, b, AdmmOptions(eps_abs=1e-8, eps_rel=1e-8, reg_rel=0.06, max_iter=1, check_every=1, adaptive_rho=False),
                            warm_x=x0[b], warm_y=y0[b])
            assert one["iters"] == port1["iters"][b] == 1 and one["status"] == port1["status"][b], (name, kind, b)
            assert np.abs(one["x"] - port1["x"][b]).max() <= 1e-9, (name, kind, b)
            assert np.abs(one["y"] - port1["y"][b]).max() <= 1e-9 * max(1.0, np.abs(port1["y"][b]).max()), (name, kind, b)
            ref = solve_one(batch, b, AdmmOptions(eps_abs=1e-8, eps_rel=1e-8, reg_rel=0.06), warm_x=x0[b], warm_y=y0[b])
            assert ref["status"] == 1 and port["status"][b] == 1, (name, kind, b)
            assert abs(int(ref["iters"]) - int(port["iters"][b])) <= 20, (name, kind, b, ref["iters"], port["iters"][b])
            assert np.abs(ref["x"] - port["x"][b]).max() <= 1e-6, (name, kind, b)


def test_numpy_restatement_refuses_half_a_warm_start():
    from oracle.admm_ref import solve_one

    batch = WC.pool("n8_soc")
    with pytest.raises(ValueError):
        solve_one(batch, 0, warm_x=WC.warm("n8_soc", "exact")[0][0])


@pytest.mark.parametrize("name,t_max", [(n, t) for n in WC.MIXED for t in (12, 13)])
def test_stale_multipliers_at_dead_periods_are_read_as_zero(name, t_max):
    """include/acn_qp.h: y is exactly zero at t >= horizon[b] for every status.  A closed loop can hand over warm_y entries
    at periods that are dead by now (the horizon shortens by more than the shift); they are read as zero: y is exactly zero
    there after 1, 20 and 60 iterations and at the end, and every output has the bits of the run from ``exact``."""
    batch = WC.pool(name)
    _, live = WC.masks(batch, t_max)
    y0 = WC.warm(name, "stale", t_max)[1]
    assert (np.abs(y0)[np.broadcast_to(~live, y0.shape)] > 0).all() and (~live).sum() >= batch.B / 3
    for run in WC.STALE_RUNS + ("full",):
        out, ref = WC.twin(name, "stale", run, t_max), WC.twin(name, "exact", run, t_max)
        assert not (out["y"] * ~live).any(), (name, run, float(np.abs(out["y"] * ~live).max()))
        assert not (out["x"] * ~live).any(), (name, run)
        for key in OUTPUTS:
            assert np.array_equal(out[key], ref[key]), (name, run, key)


@pytest.mark.parametrize("name", list(WC.POOLS))
def test_iteration_counts_that_hang_on_an_adaptation_decision(name):
    """WC.ITER_FRAGILE is exactly the set of problems whose count of a warm-started full solve the twin itself moves when the
    cost vector moves by 1e-13 relative (options_cases.ITER_FRAGILE); three of a pool at the most"""
    found = {}
    for kind in WC.FULL_KINDS:
        fr = WC.iter_fragile(name, kind)
        assert len(fr) <= 3, (name, kind, fr)
        if fr:
            found[name, kind] = fr
        assert (WC.twin(name, kind, "full")["status"] == 1).all(), (name, kind)
    assert found == {k: v for k, v in WC.ITER_FRAGILE.items() if k[0] == name}, found


def test_retry_behind_a_warm_pass_on_the_stalled_pool():
    """stall200_retry1 from ``perturbed``: pass 0 starts warm and ends on a plateau, the retry (cold, fixed penalty) runs on
    every problem; no status hangs on the deciding threshold beyond WC.RETRY_DROPPED"""
    warm, first = WC.twin("stalled", "perturbed", "retry"), WC.twin("stalled", "perturbed", "retry", retry_passes=0)
    print(f"[warm] stalled, stall200_retry1 from perturbed: statuses {warm['status'].tolist()}, iters {warm['iters'].tolist()} "
          f"(pass 0 alone {first['iters'].tolist()})")
    assert np.isin(warm["status"], (1, 2, 5)).all()
    assert (warm["iters"] > first["iters"]).all()   # the retry ran
    assert WC.fragile("stalled", "perturbed", "retry") == WC.RETRY_DROPPED
    assert len(WC.RETRY_DROPPED) <= 0.2 * WC.pool("stalled").B
