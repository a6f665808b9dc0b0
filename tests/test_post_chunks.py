"""The staging loop of the post-solve host entries (adacharge_amd/csrc/acn_qp_post.hpp: acnqp_duals_host,
acnqp_pilots_host, acnqp_advance_host) with MORE THAN ONE chunk.  ``ACNQP_POST_CHUNK`` (a diagnostic variable read at
every call) caps the chunk at a few problems, so that a call of seven problems runs as 3 + 3 + 1: the second and third
chunk take their slice of every per-problem array, read the whole-call arrays through absolute indices (``sess_seg + lo``,
``a_seg + lo``), and reuse the staging buffer.  Every output must equal BIT FOR BIT the same call with the variable unset
(one chunk) and, for advance and pilots, the specification the one-chunk tests compare against."""
import functools

import numpy as np
import pytest

from tests import advance_spec, pilots_cases
from tests import test_advance_gpu as A
from tests import test_duals_gpu as D
from tests import test_pilots_gpu as P

pytestmark = pytest.mark.gpu


def _same_dict(got, ref, what):
    assert set(got) == set(ref), what
    for k in ref:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)


# ---- advance: B = 7 at cap 3, arrivals in every chunk -------------------------------------------------------------------
@pytest.mark.parametrize("N,Tm,K", [(54, 12, 1), (70, 20, 1)])
def test_advance_in_chunks_of_3_3_1(N, Tm, K, monkeypatch):
    (c, applied, status, x, y, plan, _), want = A._case(N, Tm, K)
    seg = plan["a_seg"]
    assert len(applied) == 7 and seg[3] > 0 and seg[6] > seg[5]      # chunk two finds its records behind those of chunk one
    h = A._handle(N)
    run = lambda: h.advance(c, applied, A._plan(plan), plan["step"], status=status, x=x, y=y, want_warm=True)
    bare = lambda: h.advance(c, applied, A._plan(plan), plan["step"])   # no status, no warm outputs
    one, one_bare = run(), bare()
    monkeypatch.setenv("ACNQP_POST_CHUNK", "3")
    got, got_bare = run(), bare()
    _same_dict(got, one, "status, x, y, warm outputs")
    A._same(got, want)
    assert "warm_x" in got and "warm_y" in got and "flags" in got
    _same_dict(got_bare, one_bare, "no status, no warm outputs")
    A._same(got_bare, advance_spec.advance(c, applied, None, None, None, plan))
    assert "warm_x" not in got_bare


# ---- pilots: the first 7 snapshots of the caltech54 pool at cap 3 -------------------------------------------------------
@pytest.mark.parametrize("mode", P.MODES)
def test_pilots_in_chunks_of_3_3_1(mode, monkeypatch):
    infra, iface, table, rates = pilots_cases.pool(*pilots_cases.POOLS[0])
    plan, x = P._take(pilots_cases.plan_of(infra, iface, table, rates, mode), rates, range(7))
    want, visits = P._spec(plan, x)
    if mode == "reallocate":    # the second and the third chunk reallocate: their sessions are found through sess_seg + lo
        assert visits[3:6].max() > 0 and visits[6] > 0 and plan.sess_seg[3] > 0
    h = P._handle(infra)
    one, one_first = h.pilots(plan, x), h.pilots(plan, x, want_pilots=False)
    monkeypatch.setenv("ACNQP_POST_CHUNK", "3")
    got, got_first = h.pilots(plan, x), h.pilots(plan, x, want_pilots=False)
    h.close()
    for k in range(3):
        assert np.array_equal(got[k], one[k]), (mode, k)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want[:, :, 0]) and np.array_equal(got[2], visits), mode
    assert got_first[0] is None and one_first[0] is None
    assert np.array_equal(got_first[1], one_first[1]) and np.array_equal(got_first[2], one_first[2]), mode
    assert np.array_equal(got_first[1], want[:, :, 0]) and np.array_equal(got_first[2], visits), mode


# ---- duals: the wave form in chunks of 4, 2 and the block form in chunks of 3, 1 ----------------------------------------
@functools.lru_cache(maxsize=None)
def _batches():
    return D._shape_batches()


@pytest.mark.parametrize("name,B,cap", [("54x12_soc_eq_peak_k2", 6, 4), ("100x24_flat", 4, 3)])
def test_duals_in_chunks(name, B, cap, monkeypatch):
    from adacharge_amd.backend import SiteHandle

    batch = _batches()[name]
    assert batch.B == B and (batch.N <= 64) == (name == "54x12_soc_eq_peak_k2")
    h = SiteHandle(batch.site, 0)
    res = h.solve(batch, want_y=True)
    assert np.isin(res.status, (1, 5)).all(), res.status
    one = {wz: h.duals(batch, res, want_z=wz) for wz in (True, False)}
    monkeypatch.setenv("ACNQP_POST_CHUNK", str(cap))
    got = {wz: h.duals(batch, res, want_z=wz) for wz in (True, False)}
    h.close()
    for wz in (True, False):
        for k in ("mu", "stat", "energy", "site", "comp"):
            assert np.array_equal(getattr(got[wz], k), getattr(one[wz], k)), (name, wz, k)
    assert got[False].z is None and one[False].z is None and np.array_equal(got[True].z, one[True].z), name
    assert np.array_equal(got[False].mu, got[True].mu) and np.isfinite(got[True].stat).all()
