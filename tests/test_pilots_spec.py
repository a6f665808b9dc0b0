"""tests/pilots_spec.py -- the contract of the pilot-signal kernel -- equals the host post-processing
(postprocessing.project_into_*_batch, diff_based_reallocation_batch) exactly where no decision sits on a rounding, and
the library exports the new entries (their layout against the C header: tests/test_abi.py).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from adacharge_amd import backend, postprocessing as pp
from tests import pilots_cases as cases, pilots_spec as spec


def _spec_all(infra, iface, table, rates):
    plan = cases.plan_of(infra, iface, table, rates, "reallocate")
    return plan, spec.reallocate(rates, plan.levels, plan.cre, plan.cim, plan.limits, plan.sess_seg, plan.s_evse, plan.s_arrived, plan.s_cap)


@pytest.mark.parametrize("site_name,seed,most_visits", [(*cases.POOLS[0], 58), (*cases.POOLS[1], 53)])
def test_spec_equals_host_batch_functions_on_the_pools(site_name, seed, most_visits):
    infra, iface, table, rates = cases.pool(site_name, seed)
    plan, got, visits, margin = cases.pool_reference(site_name, seed)
    print(f"{site_name}: smallest decision margin {margin.min():.3e} A, most visits {visits.max()}")
    assert np.array_equal(spec.continuous(rates - 1.0, plan.max_pilot), pp.project_into_continuous_feasible_pilots_batch(rates - 1.0, infra))
    assert np.array_equal(spec.continuous(rates * 3.0, plan.max_pilot), pp.project_into_continuous_feasible_pilots_batch(rates * 3.0, infra))
    disc = pp.project_into_discrete_feasible_pilots_batch(rates, infra)
    assert np.array_equal(spec.discrete(rates, plan.levels), disc)
    assert np.array_equal(spec.discrete(rates - 1.0, plan.levels), pp.project_into_discrete_feasible_pilots_batch(rates - 1.0, infra))
    want = pp.diff_based_reallocation_batch(rates, table, infra, iface)
    # no snapshot may be excluded on these pools: every order-dependent decision is far from its threshold
    assert (margin >= 1e-6).all(), margin.min()
    assert np.array_equal(got, want)
    assert (got[:, :, 0] != disc[:, :, 0]).any()          # the round robin did hand rounding loss back
    assert (visits >= 0).all() and visits.max() == most_visits   # counted on this pool; the bound N L is 1404 / 1352
    two = np.bincount(table.prob * table.N + table.evse).max()
    assert two == 2                                        # EVSEs that appear twice in the visiting order are in the pool


def test_spec_equals_host_on_the_three_evse_known_answers():
    firsts = []
    for infra, iface, table, rates in cases.small_cases():
        plan, (got, visits, margin) = _spec_all(infra, iface, table, rates)
        assert np.array_equal(got, pp.diff_based_reallocation_batch(rates, table, infra, iface))
        assert np.array_equal(got[0], pp.diff_based_reallocation(rates[0].copy(), iface.active_sessions(), infra, iface))
        assert np.array_equal(spec.discrete(rates, plan.levels), pp.project_into_discrete_feasible_pilots_batch(rates, infra))
        assert np.array_equal(spec.continuous(rates, plan.max_pilot), pp.project_into_continuous_feasible_pilots_batch(rates, infra))
        assert visits[0] > 0
        firsts.append(got[0, :, 0].tolist())
    assert firsts[0] == [17, 16, 17], firsts   # t_post.py:262-280


def test_floor_to_set_count_rule_on_the_level_grid():
    """The count rule against postprocessing.floor_to_set around every rounding edge: level - 0.05 and its two
    neighbouring doubles, the level itself and its neighbours, far ends."""
    levels = np.r_[0.0, np.arange(8.0, 33.0)]
    padded = np.r_[levels, np.inf, np.inf]
    grid = [-1.0, -0.06, 40.0, 1e9, 4.0]
    for l in levels:
        for c in (l - 0.05, l, l + 0.05):
            grid += [np.nextafter(c, -np.inf), c, np.nextafter(c, np.inf)]
    for v in grid:
        want = pp.floor_to_set(v, levels)
        assert spec.floor_to_set(v, levels) == want, v
        assert spec.floor_to_set(v, padded) == want, v
    x = np.array(grid).reshape(1, 1, -1)
    assert np.array_equal(spec.discrete(x, padded[None, :])[0, 0], np.maximum(pp.floor_to_set(np.array(grid), levels), 0))


def test_endless_input_stops_at_the_bound():
    plan, rates = cases.endless_case()
    got, visits, _ = spec.reallocate(rates, plan.levels, plan.cre, plan.cim, plan.limits, plan.sess_seg, plan.s_evse, plan.s_arrived, plan.s_cap)
    assert visits[0] == -1 and np.array_equal(got, rates)
    # exactly N L visits were made: with the cap at the last level the same input retires at its first visit
    counted = []
    orig = spec.increment
    try:
        spec.increment = lambda cur, lv: (counted.append(1), orig(cur, lv))[1]
        spec.reallocate(rates, plan.levels, plan.cre, plan.cim, plan.limits, plan.sess_seg, plan.s_evse, plan.s_arrived, plan.s_cap)
    finally:
        spec.increment = orig
    assert len(counted) == plan.N * plan.levels.shape[1]
    _, v2, _ = spec.reallocate(rates, plan.levels, plan.cre, plan.cim, plan.limits, plan.sess_seg, plan.s_evse, plan.s_arrived, np.array([32.0]))
    assert v2[0] == 1


def test_library_exports_the_entries_and_refuses_a_null_handle(hip_library):
    out = backend._Pilots(None, None, None)
    plan = backend._PilotPlan()
    assert hip_library.acnqp_pilots_device(None, C.byref(plan), None, C.byref(out), None) == -1
    assert b"null handle" in hip_library.acnqp_last_error()
    assert hip_library.acnqp_pilots_host(None, C.byref(plan), None, C.byref(out)) == -1
    assert b"acnqp_pilots_host" in hip_library.acnqp_last_error()
