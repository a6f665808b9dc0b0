"""The direct path for x: with PINNED result arrays the wave kernel (one wave per problem) stores
every schedule straight into the caller's array; with pageable ones the chunk loop copies it back as before.  Every call
of tests/direct_x_cases.py is solved both ways in one process and every output must be equal bit for bit.  The pinned x is
pre-filled with NaN, so that an element nobody wrote shows, and acnqp_debug_direct_x says which path ran: the number of
problems meant to go direct, 0 for the pageable call.  ACNQP_NO_DIRECT_X=1 (read once per process: a child) gives the
same bits through the copy path."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import direct_x_cases as DC

SWITCHES = ("ACNQP_NO_DIRECT_X", "ACNQP_PLAN", "ACNQP_CHUNK", "ACNQP_NO_RAMP", "ACNQP_NO_STAGING", "ACNQP_NO_WAVE", "ACNQP_WAVE_MIN_BATCH",
            "ACNQP_NO_POLISH", "ACNQP_NO_ORDER", "ACNQP_NO_QUEUE")


def _both_ways(name, pinned=None, warm_from_cold=False):
    """the call `name` with pinned[g] (default: all pinned) and with pageable result arrays; returns (handle, outputs, what
    the two calls added to the polish counters)"""
    from adacharge_amd.backend import SiteHandle

    batches, options, warm = DC.build(name)
    pinned = [True] * len(batches) if pinned is None else pinned
    h = SiteHandle(batches[0].site, 0)
    assert h.route(batches[0].Tm, batches[0].K, sum(b.B for b in batches))[0] == "wave1"
    if warm_from_cold:
        cold = h.solve_many(batches, options, want_y=[True] * len(batches))
        warm = [(r.x.copy(), r.y.copy()) for r in cold]
    before = h.polish_stats()
    got, direct = DC.solve(h, batches, options, pinned, warm)
    assert direct == sum(b.B for b, p in zip(batches, pinned) if p), (name, direct)
    ref, none = DC.solve(h, batches, options, [False] * len(batches), warm)
    assert none == 0, name
    for k in DC.KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (name, k)
    assert not np.isnan(got["x"]).any() and not (got["status"] == 0).any(), name
    after = h.polish_stats()
    return h, got, {k: after[k] - before[k] for k in ("attempted", "solved")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1_t1", "n7_t5", "n54_t12", "n64_t12", "short_horizons"])
def test_sites_and_horizons(name):
    h, _, _ = _both_ways(name)
    h.close()


@pytest.mark.gpu
def test_pieces_of_one_batch_in_different_chunks(monkeypatch):
    from adacharge_amd.backend import SiteHandle

    monkeypatch.setenv("ACNQP_PLAN", "3,4")   # batches of 5, 1, 7 in chunks of 3, 4, 6
    h, got, _ = _both_ways("pieces")
    n0 = int(h._lib.acnqp_launch_count(h._h))
    batches, options, _ = DC.build("pieces")
    DC.solve(h, batches, options, [True] * 3)
    assert int(h._lib.acnqp_launch_count(h._h)) - n0 == 3
    h.close()
    monkeypatch.delenv("ACNQP_PLAN")
    h1 = SiteHandle(batches[0].site, 0)   # ... and the same bits as the call in one chunk
    one, direct = DC.solve(h1, batches, options, [True] * 3)
    h1.close()
    assert direct == 13
    for k in DC.KEYS:
        assert np.array_equal(got[k], one[k]), k


@pytest.mark.gpu
def test_pinned_and_pageable_batches_in_one_call(monkeypatch):
    monkeypatch.setenv("ACNQP_PLAN", "3,4")
    h, _, _ = _both_ways("pieces", pinned=[True, False, True])
    h.close()
    h, _, _ = _both_ways("pieces", pinned=[False, True, False])
    h.close()


@pytest.mark.gpu
def test_empty_set_and_infeasible_verdicts():
    h, got, _ = _both_ways("verdicts")
    h.close()
    assert got["status"].ravel().tolist() == [1, 4, 1, 3, 1]
    assert not got["x"][1].any()   # (the empty-set exit stores a schedule of zeros)


@pytest.mark.gpu
def test_handed_over_problems():
    """polish_iters = 300 hands a quarter of the problems over (63 of 256 per call; the polish solves all of them: the case of
    tests/polish_alongside_cases.py it is taken from has none that is passed on to the resume launch)"""
    h, got, polish = _both_ways("hand_over")
    h.close()
    print("two calls: handed over", polish["attempted"], "polished", polish["solved"], "passed on", polish["attempted"] - polish["solved"])
    assert polish["attempted"] >= 16 and polish["solved"] >= 2
    assert not (got["status"] == 6).any()


@pytest.mark.gpu
def test_warm_started_call():
    """the same problems and options, warm-started from their cold answers: no polish runs"""
    h, _, polish = _both_ways("hand_over", warm_from_cold=True)
    h.close()
    assert polish["attempted"] == 0


@pytest.mark.gpu
def test_launch_order_is_active():
    from adacharge_amd.backend import SiteHandle

    batches, options, _ = DC.build("launch_order")
    assert sum(b.B for b in batches) >= 768 and (batches[0].N, batches[0].Tm) == (8, 4)
    h0 = SiteHandle(batches[0].site, 0)
    n0 = h0.ordered_launches()
    _, direct = DC.solve(h0, batches, options, [True] * len(batches))
    assert h0.ordered_launches() > n0 and direct == 800
    h0.close()
    h, _, _ = _both_ways("launch_order")
    h.close()


@pytest.mark.gpu
def test_the_copy_path_everywhere_gives_the_same_bits():
    from adacharge_amd.backend import SiteHandle

    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "off.npz")
        subprocess.run([sys.executable, DC.__file__, f], check=True, env=dict(env, ACNQP_NO_DIRECT_X="1"), timeout=300)
        with np.load(f) as z:
            off = {k: z[k] for k in z.files}
    for name in DC.CHILD_CALLS:
        assert int(off[f"{name}:direct"]) == 0, name
        batches, options, warm = DC.build(name)
        h = SiteHandle(batches[0].site, 0)
        got, direct = DC.solve(h, batches, options, [True] * len(batches), warm)
        h.close()
        assert direct == sum(b.B for b in batches)
        for k in DC.KEYS:
            assert np.array_equal(got[k], off[f"{name}:{k}"]), (name, k)
