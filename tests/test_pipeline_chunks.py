"""The host-buffer entries' chunk pipeline (adacharge_amd/csrc/acn_qp_pipeline.hpp): however a call is cut into chunks --
``ACNQP_PLAN`` / ``ACNQP_CHUNK`` (diagnostic variables read at every call) or the default ramp -- and whichever entry
takes it (dense, pinned or pageable results, with a device sink; session table), every output equals BIT FOR BIT the
unchunked solve of the same problems.  Six chunks on four slots reuse two slots whose staging grows between uses.

Run as a script (``name out.npz``) it solves the warm-row case of one pool, unchunked and in chunks of 8, under the
environment it was started with and saves every output: ``ACNQP_NO_STAGING`` is read once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
from adacharge_amd.acn import InfrastructureInfo, Interface
from adacharge_amd.builder import plan_from_table
from adacharge_amd.session_table import SessionTable

QC = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
KEYS = ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")


def _plan(snaps, infra, ct="SOC", peaks=None):
    iface = Interface({"infrastructure_info": infra, "period": 5})
    plan = plan_from_table(SessionTable.from_sessions(snaps, infra), infra, iface, QC, ct, False, peaks)
    return plan, plan.expand()


def _launches(h):
    return int(h._lib.acnqp_launch_count(h._h))


def _same(ref, got, what, keys=KEYS):
    for k in keys:
        assert np.array_equal(getattr(ref, k), getattr(got, k)), (what, k)


@pytest.mark.gpu
def test_wave_route_under_an_explicit_plan_keeps_every_bit(monkeypatch):
    import torch

    from adacharge_amd.backend import SiteHandle, default_options

    infra = sites.caltech54()
    plan, batch = _plan(sites.snapshot_batch(infra, 12, 96, seed=31), infra)
    h = SiteHandle(batch.site, 0)
    assert h.route(batch.Tm, batch.K, batch.B)[0] == "wave1"
    ref = h.solve(batch, default_options(), want_y=True)
    assert (ref.status == 1).all()
    monkeypatch.setenv("ACNQP_PLAN", "8,16,8,24,8")   # + the rest (32): six chunks
    n0 = _launches(h)
    _same(ref, h.solve(batch, default_options(), want_y=True, pinned_results=True), "dense, pinned")
    assert _launches(h) - n0 == 6
    _same(ref, h.solve(batch, default_options(), want_y=True, pinned_results=False), "dense, pageable")
    _same(ref, h.solve_table(plan, default_options(), want_y=True), "table")
    sink = torch.full((batch.B, batch.N, batch.Tm), float("nan"), dtype=torch.float64, device="cuda")
    run, results = h.prepare_many([batch], pinned_results=True, x_dev_ptrs=[sink.data_ptr()])
    run(default_options())
    torch.cuda.synchronize()
    _same(ref, results[0], "dense with a device sink", keys=("x", "status", "iters", "pri_res", "dua_res", "obj"))
    assert np.array_equal(sink.cpu().numpy(), ref.x)
    h.close()


def _two_sessions_T16_peak():
    infra = sites.caltech54()
    rng = np.random.default_rng(11)
    snaps = [sites.random_sessions_general(infra, 16, rng, two_per_evse=True, min_rates=True, demand_scale=0.7) for _ in range(100)]
    peaks = [float(rng.uniform(300, 600)) if b % 2 else None for b in range(100)]
    return infra, snaps, "LINEAR", peaks, "tiled_ct1"


def _wide128_T40():
    infra = sites.wide128()
    return infra, sites.snapshot_batch(infra, 40, 100, seed=40), "SOC", None, "stream"


def _caltech54_T96():
    infra = sites.caltech54()
    return infra, sites.snapshot_batch(infra, 96, 100, seed=96), "SOC", None, "long_ws"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [_two_sessions_T16_peak, _wide128_T40, _caltech54_T96])
def test_non_wave_routes_in_chunks_of_24_keep_every_bit(case, monkeypatch):
    from adacharge_amd.backend import SiteHandle, default_options

    infra, snaps, ct, peaks, family = case()
    plan, batch = _plan(snaps, infra, ct, peaks)
    h = SiteHandle(batch.site, 0)
    assert h.route(batch.Tm, batch.K, batch.B)[0] == family and (family != "tiled_ct1" or batch.K == 2)
    ref = h.solve(batch, default_options(), want_y=True)
    monkeypatch.setenv("ACNQP_CHUNK", "24")   # 24, 24, 24, 24, 4
    n0 = _launches(h)
    _same(ref, h.solve(batch, default_options(), want_y=True), "dense")
    assert _launches(h) - n0 == 5
    _same(ref, h.solve_table(plan, default_options(), want_y=True), "table")
    h.close()


@pytest.mark.gpu
def test_non_wave_ramp_gives_both_entries_the_bits_of_the_pool_solved_alone():
    """1,800 problems of a register-resident two-slot shape: chunks of 256 / 512 / 1,024 / 8 by default."""
    from adacharge_amd.backend import SiteHandle, default_options

    n = 8
    infra = InfrastructureInfo(np.ones((1, n)), np.array([120.0]), np.zeros(n), np.full(n, 208.0), constraint_ids=["feeder"],
                               station_ids=[f"E-{i:04d}" for i in range(n)], max_pilot=np.full(n, 32.0), min_pilot=np.full(n, 8.0),
                               allowable_pilots=[np.r_[0.0, np.arange(8.0, 33.0)] for _ in range(n)], is_continuous=np.zeros(n, dtype=bool))
    rng = np.random.default_rng(8)
    pool = [sites.random_sessions_general(infra, 12, rng, two_per_evse=True, min_rates=True, demand_scale=0.7) for _ in range(32)]
    _, alone_batch = _plan(pool, infra, "LINEAR")
    plan, batch = _plan((pool * 57)[:1800], infra, "LINEAR")
    assert batch.K == 2 and batch.Tm == 12 and batch.B == 1800
    h = SiteHandle(batch.site, 0)
    assert h.route(batch.Tm, batch.K, batch.B)[0] == "tiled_ct1"
    alone = h.solve(alone_batch, default_options(), want_y=True)
    n0 = _launches(h)
    dense = h.solve(batch, default_options(), want_y=True)
    assert _launches(h) - n0 == 4
    table = h.solve_table(plan, default_options(), want_y=True)
    h.close()
    _same(dense, table, "dense against table")
    for lo in range(0, 1800, 32):
        m = min(32, 1800 - lo)
        for k in KEYS:
            assert np.array_equal(getattr(dense, k)[lo:lo + m], getattr(alone, k)[:m]), (lo, k)


# ---- the arrays no chunked case above carries: lf, dc, dfloor, warm_x, warm_y -------------------------------------------
WARM_ROW_POOLS = ("n100_t24_lf", "jpl_t28_dc")   # a flat row; a max row (tests/warm_cases.py)
CUTS = ((0, 9), (9, 13), (13, 20))               # chunks of 8: 8 | 1 + 4 + 3 | 4 -- three pieces in the middle one
CHILD_TIMEOUT = 120                               # seconds for the child process of the unstaged case


def _warm_rows(name, chunk):
    """20 problems of a warm pool as batches of 9, 4 and 7 with their warm points and want_y through ``solve_many``, with
    pinned and with pageable results; ``chunk``: ACNQP_CHUNK (None: unset).  -> {"pinned" | "pageable": {key: (20, ...)}}"""
    from adacharge_amd.backend import SiteHandle, default_options
    from tests import warm_cases

    pool = warm_cases.pool(name)
    wx, wy = warm_cases.warm(name, "perturbed")
    batches = [pool.subset(slice(a, b)) for a, b in CUTS]
    warm = [(wx[a:b], wy[a:b]) for a, b in CUTS]
    assert (pool.site.has_flat or pool.site.has_max) and pool.B >= 20
    if chunk is None:
        os.environ.pop("ACNQP_CHUNK", None)
    else:
        os.environ["ACNQP_CHUNK"] = str(chunk)
    h = SiteHandle(pool.site, 0)
    out = {}
    try:
        for tag, pinned in (("pinned", True), ("pageable", False)):
            n0 = _launches(h)
            res = h.solve_many(batches, default_options(), pinned_results=pinned, want_y=[True] * 3, warm=warm)
            assert _launches(h) - n0 == (1 if chunk is None else 3)
            out[tag] = {k: np.concatenate([np.array(getattr(r, k)) for r in res]) for k in KEYS}
    finally:
        h.close()
        os.environ.pop("ACNQP_CHUNK", None)
    return out


def _same_runs(ref, got, what):
    for tag in ("pinned", "pageable"):
        for k in KEYS:
            assert np.array_equal(ref[tag][k], got[tag][k]), (what, tag, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", WARM_ROW_POOLS)
def test_flat_max_and_warm_rows_in_chunks_of_8_keep_every_bit(name, monkeypatch):
    monkeypatch.delenv("ACNQP_CHUNK", raising=False)   # (restored whatever _warm_rows does to it)
    ref = _warm_rows(name, None)
    assert (ref["pinned"]["status"] != 0).all() and ref["pinned"]["iters"].min() >= 1   # (0: UNSET)
    _same_runs(ref, _warm_rows(name, 8), name)
    for k in KEYS:
        assert np.array_equal(ref["pinned"][k], ref["pageable"][k]), k


@pytest.mark.gpu
def test_flat_and_warm_rows_without_staging_keep_every_bit(tmp_path):
    """the per-array copies of ACNQP_NO_STAGING=1, in a fresh process (the switch is read once)"""
    name, path = WARM_ROW_POOLS[0], str(tmp_path / "unstaged.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("ACNQP_CHUNK", "ACNQP_PLAN")}
    subprocess.run([sys.executable, os.path.abspath(__file__), name, path], check=True, env=dict(env, ACNQP_NO_STAGING="1"), timeout=CHILD_TIMEOUT)
    got = np.load(path)
    for tag in ("pinned", "pageable"):
        for k in KEYS:
            assert np.array_equal(got[f"whole_{tag}_{k}"], got[f"chunks_{tag}_{k}"]), (tag, k)
    assert got["whole_pinned_x"].shape[0] == 20 and (got["whole_pinned_status"] != 0).all()   # (0: UNSET)


if __name__ == "__main__":
    runs = {"whole": _warm_rows(sys.argv[1], None), "chunks": _warm_rows(sys.argv[1], 8)}
    np.savez(sys.argv[2], **{f"{run}_{tag}_{k}": v for run, d in runs.items() for tag, r in d.items() for k, v in r.items()})
