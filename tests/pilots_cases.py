"""Inputs shared by tests/test_pilots_spec.py (CPU) and tests/test_pilots_gpu.py: the two 64-snapshot pools on the recipe
of test_postprocessing.py::test_batch_postprocessing_equals_per_snapshot, the three 3-EVSE known answers of the
reference's t_post.py, and the input on which the reference's loop never ends."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from adacharge_amd import postprocessing as pp, sites
from adacharge_amd.acn import Interface
from adacharge_amd.session_table import SessionTable
from tests.acn_testing import TestingInterface, session_generator, single_phase_single_constraint, three_phase_balanced_network

POOLS = (("caltech54", 5), ("jpl52", 6))
FINE = [np.array([0] + list(range(8, 33))) for _ in range(3)]


@lru_cache(maxsize=None)
def pool(site_name, seed, B=64, T=12):
    """(infra, interface, table, rates (B, N, T)): odd snapshots with two sessions per EVSE, row 0 at 0.03 (within eps
    of a pilot value: the floor rounds UP)."""
    infra = getattr(sites, site_name)()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(seed)
    lists = [sites.random_sessions_general(infra, T, rng, two_per_evse=(b % 2 == 1), min_rates=False, demand_scale=1.0) for b in range(B)]
    table = SessionTable.from_sessions(lists, infra)
    rates = np.zeros((B, infra.num_stations, T))
    for b, sl in enumerate(lists):
        for s in sl:
            i = infra.station_ids.index(s.station_id)
            rates[b, i, s.arrival_offset : s.arrival_offset + s.remaining_time] = rng.uniform(0, 14, size=s.remaining_time)
    rates[0, :, 0] = 0.03
    rates.setflags(write=False)
    return infra, iface, table, rates


@lru_cache(maxsize=None)
def pool_reference(site_name, seed):
    """(plan, pilots, visits, margin) of the specification's REALLOCATE on a pool: computed once per process, shared by
    the CPU and the GPU tests, never modified."""
    from tests import pilots_spec as spec

    infra, iface, table, rates = pool(site_name, seed)
    plan = plan_of(infra, iface, table, rates, "reallocate")
    out, visits, margin = spec.reallocate(rates, plan.levels, plan.cre, plan.cim, plan.limits, plan.sess_seg, plan.s_evse, plan.s_arrived, plan.s_cap)
    for a in (out, visits, margin):
        a.setflags(write=False)
    return plan, out, visits, margin


def small_cases():
    """The three 3-EVSE known answers (t_post.py:262-318): [16.9, 16.5, 16.6] under a limit of 66, the same under the
    single-phase limit 49, and three-phase 16.51 sqrt(3).  Each (infra, interface, table, rates (1, 3, 10))."""
    out = []
    for cfg in (single_phase_single_constraint(3, 66, allowable_pilots=FINE), single_phase_single_constraint(3, 49, allowable_pilots=FINE),
                three_phase_balanced_network(1, 16.51 * np.sqrt(3), allowable_pilots=FINE)):
        sessions = session_generator(3, [0] * 3, [2, 3, 4], [3.3] * 3, [3.3] * 3, [32] * 3, [0] * 3)
        iface = TestingInterface({"active_sessions": sessions, "infrastructure_info": cfg, "current_time": 0, "period": 5})
        infra = iface.infrastructure_info()
        table = SessionTable.from_sessions([iface.active_sessions()], infra)
        rates = np.full((1, 3, 10), 16.0)
        rates[0, :, 0] = [16.9, 16.5, 16.6]
        out.append((infra, iface, table, rates))
    return out


def plan_of(infra, iface, table, rates, mode):
    return pp.pilot_plan_arrays(table, infra, iface, mode, batch=rates.shape[0], t_max=rates.shape[2])


def endless_case():
    """One EVSE whose last level (32) lies below its cap (40): it is raised to 32, never refused and never retired -- the
    reference's loop does not return.  (infra-like namespace, plan for REALLOCATE, rates (1, 1, 2))."""
    from adacharge_amd.backend import PilotPlan

    levels = np.array([[0.0] + list(np.arange(8.0, 33.0))])
    plan = PilotPlan(mode=2, B=1, Tm=2, N=1, max_pilot=np.array([40.0]), levels=levels, cre=np.ones((1, 1)), cim=np.zeros((1, 1)),
                     limits=np.array([100.0]), sess_seg=np.array([0, 1], np.int32), s_evse=np.zeros(1, np.int32),
                     s_arrived=np.ones(1, np.uint8), s_cap=np.array([40.0]))
    rates = np.full((1, 1, 2), 32.0)
    return plan, rates
