"""The dual report on the GPU (acnqp_duals_device / acnqp_duals_host, csrc/acn_qp_duals.hpp) against its numpy
specification (tests/duals_spec.py), on every kernel route's own answers.

  * kernel against specification, both fed the device's own (x, y, status), on the nine padded pools of
    tests/test_route_certificate.py (all eleven routes and the polish): mu, z and the four residuals agree to
    1e-10 x max(1, |q|_inf) -- the only difference allowed is the summation order / contraction of short dot products --
    every output element is written, dead periods are exact zeros;
  * every SOLVED answer has residuals within oracle/kkt.py's constants; an infeasible problem gets zeros and +inf;
  * both instantiations and both entries on 54 x 12, 54 x 144, 512 x 48, K = 2, T_b < Tm, equality / inequality rows and
    every row type: host entry = device entry bit for bit, and the same problem gives the same bits alone and at
    positions 0 and 2,048 of a 4,096 batch;
  * the public surface: ``dual_values`` has the reference's keys, shapes and signs, its energy duals are the
    interior-point oracle's, and ``solve_table`` / ``solve_batch`` give the same ``last_duals``.

``stat`` is reported in amperes (include/acn_qp.h); oracle/kkt.py's STAT_TOL is defined on stat / max(1, |q|_inf) and is
applied to that quotient."""
import numpy as np
import pytest

from oracle import kkt
from tests import duals_spec as DS
from tests import helpers as H
from tests.test_route_certificate import POOLS, _routed

AGREE = 1e-10   # x max(1, |q|_inf)


def _device_duals(h, batch, x, y, status, want_z=True, use_status=True):
    """one launch through the device entry on the given answers, every output poisoned; host arrays (mu, z, res)"""
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = DeviceBatch(batch, "cuda:0", want_y=True)
    dev.x.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    dev.y.copy_(torch.from_numpy(np.ascontiguousarray(y)))
    dev.status.copy_(torch.from_numpy(np.ascontiguousarray(status, np.int32)))
    nan = float("nan")
    mu = torch.full((batch.B, batch.K, batch.N), nan, dtype=torch.float64, device="cuda:0")
    z = torch.full((batch.B, batch.N, batch.Tm), nan, dtype=torch.float64, device="cuda:0") if want_z else None
    res = torch.full((batch.B, 4), nan, dtype=torch.float64, device="cuda:0")
    h.duals_device(dev, mu, res, z=z, stream=torch.cuda.current_stream().cuda_stream, use_status=use_status)
    torch.cuda.synchronize()
    return mu.cpu().numpy(), (None if z is None else z.cpu().numpy()), res.cpu().numpy()


def _compare(where, batch, x, y, status, mu, z, res):
    worst = 0.0
    for b in range(batch.B):
        d = DS.duals(batch, b, x[b], y[b], status[b])
        assert not np.isnan(mu[b]).any() and not np.isnan(z[b]).any() and not np.isnan(res[b]).any(), f"{where}: problem {b} unwritten"
        if status[b] not in (1, 5):
            assert not mu[b].any() and not z[b].any() and np.isposinf(res[b]).all(), (where, b)
            continue
        tol = AGREE * max(1.0, d["qn"])
        T = int(batch.T[b])
        assert not z[b][:, T:].any(), f"{where}: problem {b} dead periods of z"
        assert not mu[b][batch.s_len[b] <= 0].any(), f"{where}: problem {b} empty slots of mu"
        e = max(float(np.abs(mu[b] - d["mu"]).max()), float(np.abs(z[b] - d["z"]).max()), float(np.abs(res[b] - d["res"]).max()))
        worst = max(worst, e / max(1.0, d["qn"]))
        assert e <= tol, (where, b, e, tol, np.abs(mu[b] - d["mu"]).max(), np.abs(z[b] - d["z"]).max(), res[b], d["res"])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_kernel_equals_specification_on_every_route(name):
    from adacharge_amd.backend import SiteHandle

    pool, runs, _, _ = _routed(name)
    h = SiteHandle(pool.site, 0)
    for fam, ((t, k), padded, out, _) in runs.items():
        where = f"{name} on {fam} (t_max {t}, K {k})"
        mu, z, res = _device_duals(h, padded, out["x"], out["y"], out["status"])
        worst = _compare(where, padded, out["x"], out["y"], out["status"], mu, z, res)
        solved = out["status"] == 1
        qs = np.array([max(1.0, float(np.abs(padded.q[b]).max())) for b in range(padded.B)])
        print(f"[duals] {where}: kernel - spec {worst:.2e} (rel |q|); SOLVED worst stat/|q| {float((res[solved, 0] / qs[solved]).max()):.2e} "
              f"energy {float(res[solved, 1].max()):.2e} site {float(res[solved, 2].max()):.2e} comp {float(res[solved, 3].max()):.2e}")
        # every SOLVED answer within the certificate's constants
        assert (res[solved, 0] / qs[solved] <= kkt.STAT_TOL).all(), (where, float((res[solved, 0] / qs[solved]).max()))
        assert (res[solved, 2] <= kkt.PRI_TOL).all(), (where, float(res[solved, 2].max()))
        assert (res[solved, 3] <= kkt.COMP_TOL).all(), (where, float(res[solved, 3].max()))
        assert (res[solved, 1] <= 1e-12).all(), (where, float(res[solved, 1].max()))
        # without z (g in the library's scratch), without status: the same mu and residuals, bit for bit
        mu2, _, res2 = _device_duals(h, padded, out["x"], out["y"], out["status"], want_z=False)
        assert np.array_equal(mu, mu2) and np.array_equal(res, res2), where
    h.close()


@pytest.mark.gpu
def test_infeasible_problem_gets_zeros_and_infinite_residuals():
    from adacharge_amd.backend import SiteHandle

    batch = H.certificate_pool("caltech54", "LINEAR", 12, 6, 77, eq=True, two=False, peak="scalar")
    batch.peak[1, :] = 1.0   # one ampere for the whole site: the energy equalities cannot be met
    h = SiteHandle(batch.site, 0)
    res = h.solve(batch, want_y=True)
    assert res.status[1] not in (1, 5) and np.isin(np.delete(res.status, 1), (1, 5)).all(), res.status
    d = h.duals(batch, res)
    assert not d.mu[1].any() and not d.z[1].any()
    assert np.isposinf([d.stat[1], d.energy[1], d.site[1], d.comp[1]]).all()
    assert np.isfinite(np.delete(d.stat, 1)).all()
    # status == NULL: every problem counts as solved
    mu, z, r = _device_duals(h, batch, res.x, res.y, res.status, use_status=False)
    assert np.isfinite(r).all()
    h.close()


def _shape_batches():
    """name -> batch: both instantiations (N <= 64: wave; else workgroup), K = 2, T_b < Tm, equality and inequality rows,
    SOC / LINEAR / peak / flat / max rows"""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch

    out = {
        "54x12_soc_eq_peak_k2": H.certificate_pool("caltech54", "SOC", 12, 6, 51, eq=True, peak="mixed"),
        "54x12_lin_k1": H.certificate_pool("caltech54", "LINEAR", 12, 6, 52, two=False, peak="vector"),
        "54x144": H.pad_batch(H.certificate_pool("caltech54", "SOC", 16, 4, 53), 144, 2),
        "100x24_flat": H.edges_pool("n100_t24_lf", 4, 3),
        "52x28_max": H.edges_pool("jpl_t28_dc", 4, 4),
    }
    infra = sites.synth512()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(54)
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
    snaps = [sites.random_sessions_general(infra, 48 - 4 * k, rng, True, False, demand_scale=0.3) for k in range(3)]
    out["512x48_k2"] = build_batch(snaps, infra, iface, obj, "SOC")
    return out


@pytest.mark.gpu
def test_both_instantiations_both_entries_same_bits():
    from adacharge_amd.backend import SiteHandle
    from adacharge_amd.builder import ProblemBatch

    seen_k2 = seen_short = False
    for name, batch in _shape_batches().items():
        h = SiteHandle(batch.site, 0)
        res = h.solve(batch, want_y=True)
        assert np.isin(res.status, (1, 5)).all(), (name, res.status)
        seen_k2 |= batch.K == 2
        seen_short |= bool((batch.T < batch.Tm).any())
        host = h.duals(batch, res)
        mu, z, r = _device_duals(h, batch, res.x, res.y, res.status)
        worst = _compare(name, batch, res.x, res.y, res.status, mu, z, r)
        print(f"[duals] {name}: N {batch.N} Tm {batch.Tm} K {batch.K}: kernel - spec {worst:.2e}")
        # host entry = device entry, bit for bit
        assert np.array_equal(host.mu, mu) and np.array_equal(host.z, z), name
        assert np.array_equal(np.stack([host.stat, host.energy, host.site, host.comp], axis=1), r), name
        # the same problems alone and at positions 0 and 2,048 of a 4,096 batch
        if name in ("54x12_soc_eq_peak_k2", "100x24_flat"):   # one shape per instantiation
            idx = np.arange(4096) % batch.B
            pos = 2048
            idx[pos:pos + batch.B] = np.arange(batch.B)
            big = batch.subset(idx)
            bmu, bz, br = _device_duals(h, big, res.x[idx], res.y[idx], res.status[idx])
            for lo in (0, pos):
                s = slice(lo, lo + batch.B)
                assert np.array_equal(bmu[s], mu) and np.array_equal(bz[s], z) and np.array_equal(br[s], r), (name, lo)
        h.close()
    assert seen_k2 and seen_short


@pytest.mark.gpu
def test_dual_values_public_surface():
    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, quick_charge
    from tests.test_duals_spec import IPM_DUAL_TOL, ipm_energy_duals, unique_sessions

    g = H.load_golden()
    infra, iface = H.caltech_interface()
    sl, meta, _ = H.golden_case(g, "c03")   # SOC, equal_share 1e-2
    assert meta["ct"] == "SOC"
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, meta["es"])]
    aco = AdaptiveChargingOptimization(obj, iface, "SOC", False)
    peak = 300.0
    rates = aco.solve(sl, infra, peak_limit=peak)
    dv = aco.dual_values(sl, infra)
    N, T = rates.shape
    # exactly the keys of the reference's constraints dict (aco.py:245-276)
    want = {"charging_rate_bounds.lb", "charging_rate_bounds.ub", "peak_constraint"}
    want |= {f"energy_constraints.{s.session_id}" for s in sl}
    want |= {f"infrastructure_constraints.{c}" for c in infra.constraint_ids}
    assert set(dv) == want
    assert dv["charging_rate_bounds.lb"].shape == (N, T) and dv["charging_rate_bounds.ub"].shape == (N, T)
    assert (dv["charging_rate_bounds.lb"] >= 0).all() and (dv["charging_rate_bounds.ub"] >= 0).all()
    assert not (dv["charging_rate_bounds.lb"] * dv["charging_rate_bounds.ub"]).any()
    assert dv["peak_constraint"].shape == (T,) and (dv["peak_constraint"] >= 0).all()
    infra_vals = np.stack([dv[f"infrastructure_constraints.{c}"] for c in infra.constraint_ids])
    assert infra_vals.shape == (len(infra.constraint_ids), T) and (infra_vals >= 0).all()
    assert infra_vals.max() > 0 or dv["peak_constraint"].max() > 0   # something binds
    assert all(dv[f"energy_constraints.{s.session_id}"] >= 0 for s in sl)   # inequality rows
    d = aco.last_duals
    assert d is aco.last_duals   # cached
    # the energy duals are the interior-point oracle's
    batch, x, y, nu = ipm_energy_duals(sl, infra, iface, meta, peak=peak)
    uniq = unique_sessions(batch, x, sl, infra)
    assert len(uniq) >= len(sl) / 2
    worst = max(abs(dv[f"energy_constraints.{sl[k].session_id}"] - nu[k]) for k, _, _ in uniq)
    print(f"[duals] dual_values vs IPM: worst {worst:.3e} over {len(uniq)} sessions, largest dual {np.abs(nu).max():.3g}")
    assert worst <= IPM_DUAL_TOL, worst
    # a binding transformer: the same case without the peak row has non-zero infrastructure duals
    aco.solve(sl, infra)
    dv2 = aco.dual_values(sl, infra)
    assert "peak_constraint" not in dv2
    assert max(dv2[f"infrastructure_constraints.{c}"].max() for c in infra.constraint_ids) > 0

    # solve_table and solve_batch give the same last_duals
    from adacharge_amd.session_table import SessionTable

    lists = [sl, H.golden_case(g, "c07")[0]]
    aco.solve_batch(lists, infra)
    a, ra = aco.last_duals, aco.last_result
    aco.solve_table(SessionTable.from_sessions(lists, infra), infra)
    b_, rb = aco.last_duals, aco.last_result
    assert a is not b_ and np.array_equal(ra.x, rb.x)
    for key in ("mu", "z", "stat", "energy", "site", "comp"):
        assert np.array_equal(getattr(a, key), getattr(b_, key)), key
    # ... and they are the report of the dense batch through the handle
    c = aco._last_handle.duals(aco.last_batch, rb, aco._last_options)
    assert np.array_equal(c.mu, b_.mu) and np.array_equal(c.z, b_.z)
