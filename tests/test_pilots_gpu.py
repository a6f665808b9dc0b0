"""The pilot-signal kernel (acnqp_pilots_device / acnqp_pilots_host) returns the bits of tests/pilots_spec.py: on the two
64-snapshot pools, the 3-EVSE known answers, a one-period batch, negative inputs and a 128-EVSE site (the workgroup
variant); the same bits alone and at any position of a batch; a counted loop on the input the reference never
returns from; and ``schedule_batch(postprocess="device")`` against the default."""
import ctypes as C

import numpy as np
import pytest

from tests import pilots_cases as cases, pilots_spec as spec

pytestmark = pytest.mark.gpu
MODES = ("continuous", "discrete", "reallocate")


def _handle(infra):
    from adacharge_amd.backend import SiteHandle
    from adacharge_amd.builder import make_site

    return SiteHandle(make_site(infra, "SOC"), 0)


def _device(h, plan, rates, want_pilots=True, want_first=True):
    """acnqp_pilots_device on NaN-poisoned outputs: (pilots, first, visits) as numpy arrays."""
    import torch

    dev = torch.device("cuda", 0)
    B, N, Tm = rates.shape
    x = torch.from_numpy(np.array(rates, dtype=np.float64)).to(dev)
    pil = torch.full((B, N, Tm), float("nan"), dtype=torch.float64, device=dev) if want_pilots else None
    first = torch.full((B, N), float("nan"), dtype=torch.float64, device=dev) if want_first else None
    visits = torch.full((B,), -7, dtype=torch.int32, device=dev)
    h.pilots_device(plan.to_device(dev), x, pilots=pil, first=first, visits=visits)
    torch.cuda.synchronize(dev)
    assert np.array_equal(x.cpu().numpy(), rates)      # the input is read only
    return (None if pil is None else pil.cpu().numpy(), None if first is None else first.cpu().numpy(), visits.cpu().numpy())


_SPEC = {}


def _spec(plan, rates):
    """The specification's (pilots, visits) for (plan, rates), computed once per input."""
    for name, seed in cases.POOLS:   # the pools' REALLOCATE reference is shared with tests/test_pilots_spec.py
        if plan.mode == 2 and rates is cases.pool(name, seed)[3] and plan.s_cap.tobytes() == cases.pool_reference(name, seed)[0].s_cap.tobytes():
            return cases.pool_reference(name, seed)[1:3]
    key = (plan.mode, rates.shape, rates.tobytes()) + tuple(None if getattr(plan, k) is None else getattr(plan, k).tobytes() for k in plan._ARRAYS)
    if key not in _SPEC:
        _SPEC[key] = _spec_now(plan, rates)
    return _SPEC[key]


def _spec_now(plan, rates):
    if plan.mode == 0:
        return spec.continuous(rates, plan.max_pilot), np.zeros(len(rates), np.int32)
    if plan.mode == 1:
        return spec.discrete(rates, plan.levels), np.zeros(len(rates), np.int32)
    cre = plan.cre if plan.cre is not None else np.zeros((0, plan.N))
    cim = plan.cim if plan.cim is not None else np.zeros((0, plan.N))
    lim = plan.limits if plan.limits is not None else np.zeros(0)
    out, visits, _ = spec.reallocate(rates, plan.levels, cre, cim, lim, plan.sess_seg, plan.s_evse, plan.s_arrived, plan.s_cap)
    return out, visits


def _check_all_modes(h, infra, iface, table, rates):
    for mode in MODES:
        plan = cases.plan_of(infra, iface, table, rates, mode)
        want, visits = _spec(plan, rates)
        pil, first, vis = _device(h, plan, rates)
        assert np.array_equal(pil, want), mode
        assert np.array_equal(first, want[:, :, 0]) and np.array_equal(first, pil[:, :, 0]), mode
        assert np.array_equal(vis, visits), mode
        hp, hf, hv = h.pilots(plan, rates)                      # the host entry: the same bits
        assert np.array_equal(hp, pil) and np.array_equal(hf, first) and np.array_equal(hv, vis), mode
        _, only_first, v2 = _device(h, plan, rates, want_pilots=False)
        assert np.array_equal(only_first, first) and np.array_equal(v2, vis), mode
    return pil, vis


@pytest.mark.parametrize("site_name,seed", cases.POOLS)
def test_device_equals_spec_on_the_pools(site_name, seed):
    infra, iface, table, rates = cases.pool(site_name, seed)
    h = _handle(infra)
    pil, vis = _check_all_modes(h, infra, iface, table, rates)
    assert vis.max() > 10 and (pil[:, :, 0] != spec.discrete(rates, cases.plan_of(infra, iface, table, rates, 1).levels)[:, :, 0]).any()
    # negative inputs, and Tm = 1 (period 0 is the whole matrix): the first 16 snapshots
    for mode in MODES:
        plan, sub = _take(cases.plan_of(infra, iface, table, rates, mode), rates, range(16))
        for x in (sub - 1.0, np.ascontiguousarray(sub[:, :, :1])):
            want, visits = _spec(plan, x)
            got, first, vis = _device(h, plan, x)
            assert np.array_equal(got, want) and np.array_equal(first, want[:, :, 0]) and np.array_equal(vis, visits), (mode, x.shape)
    h.close()


def test_device_equals_spec_on_the_three_evse_known_answers():
    firsts = []
    for infra, iface, table, rates in cases.small_cases():
        h = _handle(infra)
        pil, _ = _check_all_modes(h, infra, iface, table, rates)
        firsts.append(pil[0, :, 0].tolist())
        h.close()
    assert firsts[0] == [17, 16, 17], firsts


def test_workgroup_variant_on_a_128_evse_site():
    from adacharge_amd import sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.session_table import SessionTable

    infra = sites.wide128()
    if infra.allowable_pilots[0] is None:
        infra.allowable_pilots = [np.r_[0.0, np.arange(8.0, 33.0)] for _ in range(infra.num_stations)]
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(12)
    B, T = 8, 12
    lists = [sites.random_sessions_general(infra, T, rng, two_per_evse=(b % 2 == 1), min_rates=False, demand_scale=1.0) for b in range(B)]
    table = SessionTable.from_sessions(lists, infra)
    rates = np.zeros((B, infra.num_stations, T))
    for b, sl in enumerate(lists):
        for s in sl:
            i = infra.station_ids.index(s.station_id)
            rates[b, i, s.arrival_offset : s.arrival_offset + s.remaining_time] = rng.uniform(0, 14, size=s.remaining_time)
    h = _handle(infra)
    _, vis = _check_all_modes(h, infra, iface, table, rates)
    assert vis.max() > 10
    h.close()


def _take(plan, rates, idx):
    """The problems ``idx`` of (plan, rates) as a batch of their own."""
    from adacharge_amd.backend import PilotPlan

    idx = list(idx)
    if plan.sess_seg is None:     # CONTINUOUS, DISCRETE: nothing in the plan belongs to a problem
        return plan, np.ascontiguousarray(rates[idx])
    seg = [0]
    sel = []
    for b in idx:
        sel += list(range(int(plan.sess_seg[b]), int(plan.sess_seg[b + 1])))
        seg.append(len(sel))
    sub = PilotPlan(plan.mode, len(idx), plan.Tm, plan.N, plan.max_pilot, plan.levels, plan.cre, plan.cim, plan.limits,
                    np.array(seg, np.int32), plan.s_evse[sel], plan.s_arrived[sel], plan.s_cap[sel])
    return sub, np.ascontiguousarray(rates[list(idx)])


def test_position_invariance():
    infra, iface, table, rates = cases.pool(*cases.POOLS[0])
    plan = cases.plan_of(infra, iface, table, rates, "reallocate")
    h = _handle(infra)
    full, _, fvis = _device(h, plan, rates)
    for src in (3, 17, 40):
        solo_plan, solo_rates = _take(plan, rates, [src])
        solo, _, svis = _device(h, solo_plan, solo_rates)
        assert np.array_equal(solo[0], full[src]) and svis[0] == fvis[src]
        for pos in (0, 31, 63):
            idx = list(range(64))
            idx[pos] = src
            p2, r2 = _take(plan, rates, idx)
            got, _, vis = _device(h, p2, r2)
            assert np.array_equal(got[pos], solo[0]) and vis[pos] == svis[0], (src, pos)
    h.close()


def _endless_among_solvable():
    """The caltech54 pool with one problem made endless: an arrived session whose cap (40) lies above the last level (32),
    its EVSE solved at 32.0."""
    infra, iface, table, rates = cases.pool(*cases.POOLS[0])
    plan, rates = _take(cases.plan_of(infra, iface, table, rates, "reallocate"), rates, range(8))
    k = 5
    s = next(s for s in range(int(plan.sess_seg[k]), int(plan.sess_seg[k + 1])) if plan.s_arrived[s])
    plan.s_cap = plan.s_cap.copy()
    plan.s_cap[s] = 40.0
    rates = rates.copy()
    rates[k, plan.s_evse[s], 0] = 32.0
    return infra, plan, rates, k


def test_endless_problem_is_stopped_and_leaves_its_neighbours_alone():
    infra, plan, rates, k = _endless_among_solvable()
    want, visits = _spec(plan, rates)
    assert visits[k] == -1 and (np.delete(visits, k) >= 0).all()
    h = _handle(infra)
    got, first, vis = _device(h, plan, rates)                   # the call returns
    assert vis[k] == -1 and np.array_equal(vis, visits) and np.array_equal(got, want) and np.array_equal(first, want[:, :, 0])
    for nb in (k - 1, k + 1):
        sp, sr = _take(plan, rates, [nb])
        solo, _, svis = _device(h, sp, sr)
        assert np.array_equal(solo[0], got[nb]) and svis[0] == vis[nb]
    # the specification's own one-EVSE input: exactly N L visits, then -1
    h.close()
    from adacharge_amd.acn import InfrastructureInfo

    eplan, erates = cases.endless_case()
    one = InfrastructureInfo(np.ones((1, 1)), [100.0], [0.0], [208.0], max_pilot=[40.0], allowable_pilots=[eplan.levels[0]])
    h1 = _handle(one)
    ewant, evis = _spec(eplan, erates)
    egot, _, gvis = _device(h1, eplan, erates)
    assert evis[0] == -1 and gvis[0] == -1 and np.array_equal(egot, ewant)
    h1.close()


def test_schedule_batch_raises_on_an_endless_snapshot():
    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface

    infra = sites.caltech54()
    infra.allowable_pilots = [np.r_[0.0, np.arange(8.0, 17.0)] for _ in range(infra.num_stations)]   # end at 16 A; caps reach 32 A
    iface = Interface({"infrastructure_info": infra, "period": 5})
    alg = AdaptiveSchedulingAlgorithm([ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)], quantize=True,
                                      reallocate=True, solver_options={})
    alg.register_interface(iface)
    table = sites.snapshot_table(infra, 12, 8, seed=3)
    with pytest.raises(ValueError, match=r"snapshot \d+, EVSE CT-\d+: allowable pilots end below the session's cap"):
        alg.schedule_batch(table, postprocess="device", as_arrays=True)


def test_entry_validation():
    from adacharge_amd import backend

    infra, iface, table, rates = cases.small_cases()[0]
    h = _handle(infra)
    lib = backend.load_library()
    plan = cases.plan_of(infra, iface, table, rates, "reallocate")
    x = np.ascontiguousarray(rates)
    pil, first = np.zeros_like(x), np.zeros(x.shape[:2])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(handle, p, out):
        return lib.acnqp_pilots_host(handle, C.byref(p), ptr(x), C.byref(out)), lib.acnqp_last_error().decode()

    good = backend._Pilots(ptr(pil), ptr(first), None)
    assert call(h._h, plan._struct(), good)[0] == 0
    rc, msg = call(None, plan._struct(), good)
    assert rc == -1 and "null handle" in msg
    p = plan._struct()
    p.n_evse = 4
    rc, msg = call(h._h, p, good)
    assert rc == -1 and "n_evse" in msg
    for bad_mode in (-1, 3):
        p = plan._struct()
        p.mode = bad_mode
        rc, msg = call(h._h, p, good)
        assert rc == -1 and "mode" in msg
    rc, msg = call(h._h, plan._struct(), backend._Pilots(None, None, None))
    assert rc == -1 and "no output" in msg
    rc, msg = call(h._h, plan._struct(), backend._Pilots(ptr(x), None, None))
    assert rc == -1 and "aliases x" in msg
    # the device entry refuses the same four before any device work (so host addresses are never touched)
    def dcall(handle, p, out):
        return lib.acnqp_pilots_device(handle, C.byref(p), ptr(x), C.byref(out), None), lib.acnqp_last_error().decode()

    rc, msg = dcall(None, plan._struct(), good)
    assert rc == -1 and "null handle" in msg and "acnqp_pilots_device" in msg
    p = plan._struct()
    p.n_evse = 4
    rc, msg = dcall(h._h, p, good)
    assert rc == -1 and "n_evse" in msg
    for bad_mode in (-1, 3):
        p = plan._struct()
        p.mode = bad_mode
        rc, msg = dcall(h._h, p, good)
        assert rc == -1 and "mode" in msg
    rc, msg = dcall(h._h, plan._struct(), backend._Pilots(None, None, None))
    assert rc == -1 and "no output" in msg
    import torch

    with pytest.raises(ValueError, match="x must be a contiguous"):   # a host tensor never reaches the kernel
        h.pilots_device(plan, torch.from_numpy(x.copy()), first=torch.zeros(x.shape[:2], dtype=torch.float64))
    with pytest.raises(ValueError, match="no output"):
        h.pilots(plan, x, want_pilots=False, want_first=False)
    h.close()


@pytest.mark.parametrize("reallocate", [False, True])
def test_schedule_batch_on_the_device_equals_the_default(reallocate):
    from adacharge_amd import AdaptiveSchedulingAlgorithm, ObjectiveComponent, equal_share, postprocessing as pp, quick_charge, sites
    from adacharge_amd import session_table as st
    from adacharge_amd.acn import Interface

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    alg = AdaptiveSchedulingAlgorithm([ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)], quantize=True,
                                      reallocate=reallocate, solver_options={})
    alg.register_interface(iface)
    table = sites.snapshot_table(infra, 12, 64)
    want, wstat = alg.schedule_batch(table, as_arrays=True)
    got, gstat = alg.schedule_batch(table, postprocess="device", as_arrays=True)
    assert np.array_equal(wstat, gstat) and got.shape == want.shape
    first, fstat = alg.schedule_batch(table, postprocess="device", as_arrays=True, first_period_only=True)
    assert first.shape == want.shape[:2] and np.array_equal(first, got[:, :, 0]) and np.array_equal(fstat, gstat)
    host_first, _ = alg.schedule_batch(table, as_arrays=True, first_period_only=True)
    assert np.array_equal(host_first, want[:, :, 0])
    dicts = alg.schedule_batch(table, postprocess="device")
    ok = np.flatnonzero(np.isin(gstat, (1, 5)))
    assert all(np.array_equal(np.array([dicts[b][s] for s in infra.station_ids]), got[b][:, : len(dicts[b][infra.station_ids[0]])]) for b in ok[:4])
    if not reallocate:
        assert np.array_equal(got, want)
        return
    # the solved schedules again (the solve is deterministic): the specification's bits and its margin per snapshot
    res, _ = alg._optimizer().solve_table(st.enforce_pilot_limit(table, infra), infra, [None] * table.B, iface.get_prev_peak())
    plan = pp.pilot_plan_arrays(st.enforce_pilot_limit(table, infra), infra, iface, "reallocate", t_max=res.x.shape[2])
    sp, visits, margin = spec.reallocate(res.x, plan.levels, plan.cre, plan.cim, plan.limits, plan.sess_seg, plan.s_evse, plan.s_arrived, plan.s_cap)
    assert np.array_equal(got, sp)                              # the device equals the specification on every snapshot
    clear = margin >= 1e-9
    print(f"snapshots under the 1e-9 A margin: {int((~clear).sum())} of {len(clear)}; smallest margin {margin.min():.3e} A; "
          f"host differs from the device on {int((got != want).any(axis=(1, 2)).sum())}")
    assert (~clear).sum() <= 0.05 * len(clear)
    assert np.array_equal(got[clear], want[clear])
