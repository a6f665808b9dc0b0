"""tests/hold_spec.py checks itself -- the flags of S2 and H3, m = 0 and m = B, the order of the two comparisons of H2 on
hand-made values, select-then-hold as the identity -- and ``FleetTable.resolve_rows`` / ``resolve_plan`` are held to rules
E0 - E3: on the six fleets of the closed-loop tests (counts computed on the CPU from their arrivals and departures) and
on a hand-written fleet of three records.  No GPU."""
import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.rollout import FleetTable
from tests import helpers, hold_spec as spec

B, N, TM, K, MG = 5, 3, 4, 1, 2


def _state(rng, peak=True):
    cur = dict(horizon=rng.integers(1, TM + 1, B).astype(np.int32), lb=rng.uniform(0, 1, (B, N, TM)), ub=rng.uniform(8, 32, (B, N, TM)),
               q=rng.normal(size=(B, N, TM)), pdiag=rng.uniform(0, 1, B), s_off=rng.integers(0, 2, (B, K, N)).astype(np.int32),
               s_len=rng.integers(0, 3, (B, K, N)).astype(np.int32), s_cap=rng.uniform(0, 99, (B, K, N)), s_eq=np.ones(B, np.uint8),
               lf=rng.uniform(0, 1, B), dc=rng.uniform(0, 1, B), dfloor=rng.uniform(0, 9, B))
    if peak:
        cur["peak"] = rng.uniform(40, 90, (B, TM))
        cur["peak"][1, 2] = np.inf
    return cur


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def test_select_copies_rows_and_flags_a_bad_index():
    rng = np.random.default_rng(0)
    cur = _state(rng)
    wx, wy = rng.normal(size=(B, N, TM)), rng.normal(size=(B, MG, TM))
    keep = {k: v.copy() for k, v in cur.items()}
    idx = np.array([0, 3, 7, -1, 4], np.int32)
    out = spec.select(cur, idx, wx, wy)
    assert list(out["flags"]) == [0, 0, 1, 1, 0] and out["flags"].dtype == np.int32
    for j, b in ((0, 0), (1, 3), (4, 4)):                                   # S1
        for k in cur:
            assert out[k].dtype == cur[k].dtype and np.array_equal(_bits(out[k][j]), _bits(cur[k][b])), k
        assert np.array_equal(out["warm_x"][j], wx[b]) and np.array_equal(out["warm_y"][j], wy[b])
    for j in (2, 3):                                                        # S2: the empty problem of DeviceBatch.empty
        assert out["horizon"][j] == 1 and np.isposinf(out["peak"][j]).all() and out["s_eq"][j] == 0 and out["dfloor"][j] == 0
        for k in ("lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap", "lf", "dc", "warm_x", "warm_y"):
            assert not np.any(out[k][j]), k
    assert all(np.array_equal(_bits(cur[k]), _bits(keep[k])) for k in cur)  # nothing given is changed
    # without a peak row, without a warm start: those arrays are not there
    out = spec.select(_state(rng, peak=False), idx[:2])
    assert "peak" not in out and "warm_x" not in out and "warm_y" not in out
    # m = 0 and m = B
    none = spec.select(cur, np.zeros(0, np.int32), wx, wy)
    assert none["lb"].shape == (0, N, TM) and none["flags"].shape == (0,) and none["warm_y"].shape == (0, MG, TM)
    every = spec.select(cur, np.arange(B, dtype=np.int32), wx, wy)
    assert all(np.array_equal(_bits(every[k]), _bits(cur[k])) for k in cur) and not every["flags"].any()
    # a problem's output does not depend on j or m
    one, many = spec.select(cur, np.array([3], np.int32), wx, wy), spec.select(cur, idx, wx, wy)
    assert all(np.array_equal(_bits(one[k][0]), _bits(many[k][1])) for k in one)


def test_the_clip_is_two_comparisons_in_this_order():
    clip = spec.clip
    assert clip(5.0, 0.0, 3.0) == 3.0 and clip(-1.0, 0.0, 3.0) == 0.0 and clip(2.0, 0.0, 3.0) == 2.0
    assert np.signbit(clip(-0.0, 0.0, 3.0)) and clip(-0.0, 0.0, 3.0) == 0.0   # -0.0 < 0.0 is false: the element stays what it was
    assert not np.signbit(clip(0.0, -0.0, 3.0))
    assert clip(7.5, 0.0, 0.0) == 0.0 and not np.signbit(clip(7.5, 0.0, 0.0))  # a retired window: ub = 0 (advance rule 3)
    assert np.signbit(clip(7.5, 0.0, -0.0))                                    # the value that comes out is ub itself
    assert clip(4.0, 6.0, 3.0) == 6.0                                          # lb above ub: the second comparison has the last word
    assert clip(1e300, 0.0, np.inf) == 1e300


def test_hold_takes_rows_holds_the_rest_and_flags_a_bad_row():
    rng = np.random.default_rng(1)
    m = 2
    lb, ub = np.zeros((B, N, TM)), np.full((B, N, TM), 32.0)
    ub[1, 2, :] = 0.0                                                       # a session the advance retired early
    held_x, held_y = rng.uniform(-1, 40, (B, N, TM)), rng.normal(size=(B, MG, TM))
    held_x[1, 0, 0] = -0.0
    rx, ry = rng.uniform(0, 32, (m, N, TM)), rng.normal(size=(m, MG, TM))
    rstatus, riters = np.array([1, 3], np.int32), np.array([70, 900], np.int32)
    prev = np.array([1, 2, 5, 1, 1], np.int32)
    pos = np.array([-1, -1, 0, 7, 1], np.int32)                             # 7: neither -1 nor a row
    out = spec.hold(pos, m, rx, rstatus, riters, held_x, prev, lb, ub, ry, held_y)
    assert list(out["solved"]) == [0, 0, 1, 0, 1] and out["solved"].dtype == np.uint8
    assert list(out["flags"]) == [0, 0, 0, spec.HOLD_BAD_ROW, 0]
    assert list(out["status"]) == [1, 2, 1, 1, 3] and list(out["iters"]) == [0, 0, 70, 0, 900]
    assert np.array_equal(out["x"][2], rx[0]) and np.array_equal(out["x"][4], rx[1])            # H1
    assert np.array_equal(out["y"][2], ry[0]) and np.array_equal(out["y"][4], ry[1])
    for b in (0, 1, 3):                                                                           # H2 (and H3: held all the same)
        assert np.array_equal(out["x"][b], np.where(held_x[b] > ub[b], ub[b], np.where(held_x[b] < lb[b], lb[b], held_x[b])))
        assert (out["x"][b] >= lb[b]).all() and (out["x"][b] <= ub[b]).all() and np.array_equal(out["y"][b], held_y[b])
    assert np.signbit(out["x"][1, 0, 0]) and not out["x"][1, 2].any() and (held_x[1, 2] > 0).any()
    # m = 0: everyone is held, nothing of the dense results is read
    all_held = spec.hold(np.full(B, -1, np.int32), 0, None, None, None, held_x, prev, lb, ub, None, held_y)
    assert not all_held["solved"].any() and not all_held["flags"].any() and np.array_equal(all_held["status"], prev)
    assert not all_held["iters"].any() and np.array_equal(all_held["y"], held_y)
    assert "y" not in spec.hold(pos, m, rx, rstatus, riters, held_x, prev, lb, ub)


def test_select_then_hold_with_identical_results_is_the_identity_on_x():
    rng = np.random.default_rng(2)
    cur = _state(rng)
    x = rng.uniform(cur["lb"], cur["ub"])                                   # a solver output: inside the bounds
    x[0, 0, 0], cur["lb"][0, 0, 0] = -0.0, 0.0
    y = rng.normal(size=(B, MG, TM))
    status = np.array([1, 5, 1, 2, 1], np.int32)
    for idx in ([], [2], [0, 2, 4], [0, 1, 2, 3, 4]):
        idx = np.array(idx, np.int32)
        dense = spec.select(cur, idx, x, y)                                 # "results" that are the held schedule itself
        pos = spec.inverse(idx, B)
        assert all(pos[b] == j for j, b in enumerate(idx)) and (pos >= 0).sum() == len(idx)
        out = spec.hold(pos, len(idx), dense["warm_x"], status[idx], np.full(len(idx), 9, np.int32), x, status, cur["lb"], cur["ub"],
                        dense["warm_y"], y)
        assert np.array_equal(_bits(out["x"]), _bits(x)) and np.array_equal(_bits(out["y"]), _bits(y))
        assert np.array_equal(out["status"], status) and np.array_equal(out["solved"].astype(bool), pos >= 0)
        assert np.array_equal(out["iters"], np.where(pos >= 0, 9, 0)) and not out["flags"].any()


# ---- the mask ----------------------------------------------------------------------------------------------------------
STEPS = 26


def _table():
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    rng = np.random.default_rng(77)
    fleets = [helpers.closed_loop_fleet(infra, rng, n_evs=5, t_span=14, stay=(8, 13)) for _ in range(6)]
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    return fleets, FleetTable([[dict(e, max_rate=32.0) for e in f] for f in fleets], infra, iface, obj, STEPS, t_max=12, peak_limit=40.0)


@pytest.mark.parametrize("max_recompute,share,nobody,everybody,one", [(None, 0.33, 5, 2, 7), (4, 0.42, 2, 2, 2)])
def test_mask_of_the_closed_loop_fleets(max_recompute, share, nobody, everybody, one):
    fleets, table = _table()
    mask = table.resolve_rows(max_recompute)
    assert mask.shape == (STEPS, 6) and mask.dtype == bool and mask[0].all()
    # the rules, restated from the fleets' own arrivals and departures
    want = np.zeros((STEPS, 6), bool)
    for b, f in enumerate(fleets):
        last = None
        for s in range(STEPS):
            event = s == 0 or any(s in (e["arrival"], e["departure"]) for e in f)
            want[s, b] = event or (max_recompute is not None and s - last >= max_recompute)
            if want[s, b]:
                last = s
    assert np.array_equal(mask, want)
    count = mask.sum(axis=1)
    print(f"[resolve mask] max_recompute={max_recompute}: share {mask.mean():.4f}, nobody {int((count == 0).sum())}, "
          f"all six {int((count == 6).sum())}, exactly one {int((count == 1).sum())} of {STEPS} steps")
    assert round(float(mask.mean()), 2) == share
    assert ((count == 0).sum(), (count == 6).sum(), (count == 1).sum()) == (nobody, everybody, one)
    assert 1 - mask.mean() >= 0.5 and nobody >= 1 and everybody >= 1 and one >= 1
    if max_recompute is not None:                                           # E3: never more than max_recompute periods without a solve
        for b in range(6):
            at = np.flatnonzero(mask[:, b])
            assert np.diff(at).max() <= max_recompute and STEPS - at[-1] <= max_recompute


def test_mask_with_max_recompute_one_is_all_true():
    _, table = _table()
    assert table.resolve_rows(1).all()
    plan = table.resolve_plan(1)
    assert plan.counts() == [6] * STEPS and np.array_equal(plan.pos, np.tile(np.arange(6, dtype=np.int32), (STEPS, 1)))


def test_mask_rules_on_a_hand_written_fleet():
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "current_time": 0})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    sid = infra.station_ids
    steps, start = 12, 10
    fleet = [dict(station=sid[0], arrival=7, departure=13, requested=3.0, max_rate=32.0),     # arrives before start_time
             dict(station=sid[1], arrival=15, departure=40, requested=3.0, max_rate=32.0),    # departs beyond the run
             dict(station=sid[2], arrival=18, departure=20, requested=0.0, max_rate=32.0)]    # never admitted: it still raises events
    table = FleetTable([fleet, []], infra, iface, obj, steps, start_time=start, t_max=30)
    assert len(table._stays) == 2 and table.windows[0] == [(0, 0, 3), (1, 5, 30), (2, 8, 10)]
    on = lambda mask, b: list(np.flatnonzero(mask[:, b]))
    m = table.resolve_rows(None)
    assert on(m, 0) == [0, 3, 5, 8, 10]     # E0; unplug of the first; plug-in of the second (its unplug is beyond the run); both of the third
    assert on(m, 1) == [0]                  # an empty fleet: E0 only
    m = table.resolve_rows(3)
    assert on(m, 0) == [0, 3, 5, 8, 10]     # no gap reaches 3 but 10 -> 12, which is the end of the run
    assert on(m, 1) == [0, 3, 6, 9]         # E3 counts from the last solve
    m = table.resolve_rows(2)
    assert on(m, 0) == [0, 2, 3, 5, 7, 8, 10] and on(m, 1) == [0, 2, 4, 6, 8, 10]
    assert table.resolve_rows(np.int64(2)).sum() == m.sum()


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, "3"])
def test_max_recompute_is_none_or_a_positive_integer(bad):
    _, table = _table()
    with pytest.raises(ValueError, match="max_recompute must be None or an integer >= 1"):
        table.resolve_rows(bad)
    with pytest.raises(ValueError, match="max_recompute"):
        table.resolve_plan(bad)


@pytest.mark.parametrize("max_recompute", [None, 4])
def test_resolve_plan_is_the_mask_as_index_lists(max_recompute):
    _, table = _table()
    mask, plan = table.resolve_rows(max_recompute), table.resolve_plan(max_recompute)
    assert plan.sel_seg.dtype == plan.sel_idx.dtype == plan.pos.dtype == np.int32
    assert plan.sel_seg.shape == (STEPS + 1,) and plan.pos.shape == (STEPS, 6) and len(plan.sel_idx) == mask.sum() == plan.sel_seg[-1]
    assert plan.counts() == list(mask.sum(axis=1))
    for s in range(STEPS):
        idx = plan.sel_idx[plan.sel_seg[s]: plan.sel_seg[s + 1]]
        assert np.array_equal(idx, np.flatnonzero(mask[s])) and (np.diff(idx) > 0).all()     # ascending within the step
        assert all(plan.pos[s, b] == j for j, b in enumerate(idx))                            # pos[s, sel_idx[j]] == j
        assert (plan.pos[s][~mask[s]] == -1).all()                                            # and -1 elsewhere
        assert np.array_equal(plan.pos[s], spec.inverse(idx, 6))
