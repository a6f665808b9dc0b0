"""The reference of tests/test_options_gpu.py alone (CPU): the option sets of tests/options_cases.py on oracle/admm_port.

  * every option set is told apart from its neighbour by the twin, on at least half of a pool, by what the GPU test
    asserts there -- an option a kernel ignored could otherwise pass;
  * the status of a problem that ends at an iteration limit or on a plateau counts only where it does not hang on the
    deciding threshold (options_cases.DROPPED, at most a tenth of a pool);
  * oracle/admm_ref (readable numpy) agrees with the twin under non-default options as tests/test_admm_ref.py requires
    at the defaults."""
import numpy as np
import pytest

from tests import helpers as H
from tests import options_cases as OC

MIN_SHARE = 0.5


def _distance(a, b):
    return np.abs(a["x"] - b["x"]).reshape(len(a["iters"]), -1).max(axis=1)


def _told_apart(pool, variant, limit, x_tol, iter_bound):
    """per problem: the twin's outputs under ``variant`` differ from its neighbour's by more than the GPU test allows
    between a kernel and the twin -- status; iteration count beyond twice ``iter_bound``; schedule beyond ten ``x_tol``
    (None: the GPU test does not compare schedules there)"""
    a = OC.twin(pool, variant, **OC.base_of(limit))
    b = OC.twin(pool, OC.NEIGHBOUR.get(variant, "defaults"), **OC.base_of(limit))
    apart = (a["status"] != b["status"]) | (np.abs(a["iters"] - b["iters"]) > 2 * iter_bound)
    d = _distance(a, b)
    if x_tol is not None:
        apart |= d > 10.0 * x_tol
    return apart, d


def test_padding_leaves_the_twin_alone():
    """dead periods and empty session slots change no bit of the twin's answer: the shares below, computed at a pool's
    own shape, hold at every padded shape the GPU test launches"""
    for name, shape in (("n8_soc", (13, 2)), ("n8_soc", (49, 1)), ("pods18_lin", (17, 2)), ("stalled", (25, 5))):
        own, padded = OC.twin(name, "alpha1.0"), OC.twin(name, "alpha1.0", *shape)
        assert np.array_equal(own["status"], padded["status"]) and np.array_equal(own["iters"], padded["iters"]), (name, shape)
        for key in ("x", "y"):
            assert np.array_equal(H.pad_result(own[key], shape[0]), padded[key]), (name, shape, key)
        for key in ("pri_res", "dua_res", "obj"):
            assert np.array_equal(own[key], padded[key]), (name, shape, key)


@pytest.mark.parametrize("pool", list(OC.LAYER_A))
def test_layer_a_tells_every_set_apart(pool):
    """truncated trajectories: all end at the limit with the neighbour's count, so the iterate (or the status) must differ.
    Also the cap on TRAJ_TOL: a tenth of the smallest told-apart distance (the median distance of a pairing is the
    distance at which half of the pool is still told apart)."""
    smallest = np.inf
    for variant, limit in OC.layer_a_runs(pool)[1:]:
        apart, d = _told_apart(pool, variant, limit, OC.TRAJ_TOL, limit)
        print(f"[options] A {pool:11s} {variant:13s} limit {limit:3d}: told apart {apart.mean():.2f}, median |x - x_neighbour| {np.median(d):.2e} A")
        assert apart.mean() >= MIN_SHARE, (pool, variant, limit, apart.mean())
        smallest = min(smallest, float(np.median(d)))
    print(f"[options] A {pool}: smallest told-apart distance {smallest:.2e} A, TRAJ_TOL {OC.TRAJ_TOL:.1e} A")
    assert OC.TRAJ_TOL <= smallest / 10.0, (pool, smallest)


def _layer_b_shares():
    out = {}
    for pool in OC.LAYER_B:
        for variant in OC.COMMON_B if pool != "ct54_lp" else OC.LAYER_B[pool] + ("reg0.5",):
            bound = OC.ITER_BOUND_PERIODS * OC.check_period(variant)
            apart, _ = _told_apart(pool, variant, None, OC.RATE_TOL if pool == "ct54_lp" else None, bound)
            apart[list(OC.ITER_FRAGILE.get((pool, variant), ()))] = False   # (their count is not held to the bound)
            out[variant, pool] = float(apart.mean())
    return out


def test_layer_b_tells_every_set_apart():
    """full solves: LAYER_B lists a pairing exactly where the twin tells half of the pool apart, and every set has a pool"""
    shares = _layer_b_shares()
    for (variant, pool), share in sorted(shares.items()):
        listed = variant in OC.LAYER_B[pool]
        print(f"[options] B {pool:11s} {variant:13s}: told apart {share:.2f}{'' if listed else '  (left out)'}")
        assert listed == (share >= MIN_SHARE), (variant, pool, share)
        if not listed:
            assert abs(OC.LAYER_B_LEFT_OUT[variant, pool] - share) <= 0.0051, (variant, pool, share)   # (recorded to two decimals)
    for variant in OC.COMMON_B + OC.LAYER_B["ct54_lp"]:
        assert any(variant in vs for vs in OC.LAYER_B.values()), variant


@pytest.mark.parametrize("pool,sets", [("stalled", OC.STALL_SETS), ("n8_soc", OC.FLOOR_SETS), ("n8_soc", OC.RETRY_SETS)])
def test_stall_retry_and_floor_sets_are_told_apart(pool, sets):
    """one check period per pass (three at the most) bounds the count; the retry_rho pair is told by the iterate alone"""
    for variant in sets:
        x_tol = OC.TRAJ_TOL if variant.startswith("retry_rho") else None
        apart, d = _told_apart(pool, variant, None, x_tol, 3 * OC.ITER_BOUND_PERIODS * OC.check_period(variant))
        print(f"[options] B {pool:11s} {variant:26s} against {OC.NEIGHBOUR.get(variant, 'defaults'):22s}: told apart {apart.mean():.2f}")
        assert apart.mean() >= MIN_SHARE, (pool, variant, apart.mean())
    if "retry_rho0.5" in sets:
        a, b = (OC.twin(pool, v, **OC.LAYER_B_BASE) for v in ("retry_rho0.5", "retry_rho0.2"))
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"])   # the iterate alone
        none = OC.twin(pool, "retry_rho0.5", retry_passes=0, **OC.LAYER_B_BASE)
        assert (none["status"] == 2).all() and (a["status"] == 5).all()   # the retry pass is what is kept


def test_what_the_twin_gives_the_retry_and_floor_sets():
    """the figures tests/test_options_gpu.py relies on"""
    t = lambda v: OC.twin("n8_soc", v, **OC.LAYER_B_BASE)
    assert (t("short100_floor0")["status"] == 2).all() and (t("short100_floor1e-2")["status"] == 5).all()
    assert np.bincount(t("short100_floor_default")["status"], minlength=6).tolist() == [0, 0, 23, 0, 0, 1]
    first = t("retry_stall0")
    unsolved = first["status"] != 1
    assert 0.4 <= unsolved.mean() <= 0.8 and (first["iters"][unsolved] == 240).all() and (first["iters"][~unsolved] <= 240).all()
    for variant, total in (("retry2_140", 380), ("retry2_400", 720), ("retry1_400", 480)):
        it = t(variant)["iters"]
        assert (it[unsolved] == total).all() and np.array_equal(it[~unsolved], first["iters"][~unsolved]), (variant, it)
    hist = lambda v: np.bincount(OC.twin("stalled", v, **OC.LAYER_B_BASE)["status"], minlength=6)[[1, 2, 5]].tolist()
    assert hist("defaults") == [4, 0, 6] and hist("stall200") == [2, 0, 8] and hist("stall200_retry1") == [0, 4, 6]
    assert hist("noretry_floor1e-3_stall200") == [0, 0, 10] and hist("noretry_floor0") == [2, 4, 4]


@pytest.mark.parametrize("pool", list(OC.LAYER_B))
def test_iteration_counts_that_hang_on_an_adaptation_decision(pool):
    """ITER_FRAGILE is exactly the set of problems whose count the twin itself moves when the cost vector moves by 1e-13
    relative; three of a pool at the most"""
    found = {}
    for p, variant in OC.full_solve_runs():
        if p != pool:
            continue
        fr = OC.iter_fragile(pool, variant, **OC.LAYER_B_BASE)
        if fr:
            found[pool, variant] = fr
        assert len(fr) <= 3, (pool, variant, fr)
    assert found == {k: v for k, v in OC.ITER_FRAGILE.items() if k[0] == pool}, found


def test_classification_probes_are_robust():
    """DROPPED is exactly the set of problems whose status at a limit hangs on the deciding threshold, a tenth of a pool
    at the most in any run"""
    found = {}
    for pool, variant, limit in OC.limit_runs():
        fr = OC.fragile(pool, variant, **OC.base_of(limit))
        if fr:
            found[pool, variant, limit] = fr
        assert len(fr) <= 0.1 * OC.pool(pool).B, (pool, variant, limit, fr)
    assert found == OC.DROPPED, found


GROUND = {   # variant -> the same option set in oracle/admm_ref.AdmmOptions (adapt_every = 0 is adaptive_rho = False there)
    "alpha1.0": dict(alpha=1.0),
    "sigma1e-3": dict(sigma=1e-3),
    "rho0.2_fixed": dict(rho=0.2, adaptive_rho=False),
    "ce7_ae7": dict(check_every=7, adapt_every=7),
}


@pytest.mark.parametrize("variant", list(GROUND))
def test_numpy_restatement_grounds_the_twin_under_the_options(variant):
    """As tests/test_admm_ref.py::test_numpy_twin_and_c_port_run_the_same_algorithm at the defaults: both solve, iteration
    counts within 20, schedules within 1e-6 A -- on two problems of n8_soc.  AdmmOptions has every field these four sets
    use; it has no stall window, retry passes or inaccurate floor (constants there), which these sets leave alone."""
    from oracle.admm_ref import AdmmOptions, solve_one

    batch = OC.pool("n8_soc")
    port = OC.twin("n8_soc", variant, **OC.LAYER_B_BASE)
    for b in (0, 1):
        ref = solve_one(batch, b, AdmmOptions(eps_abs=1e-8, eps_rel=1e-8, reg_rel=0.06, accel_mem=0, **GROUND[variant]))
        assert ref["status"] == 1 and port["status"][b] == 1
        assert abs(int(ref["iters"]) - int(port["iters"][b])) <= 20
        assert np.abs(ref["x"] - port["x"][b]).max() <= 1e-6
