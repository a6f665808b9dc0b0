"""``vjp_long_kernel`` (adacharge_amd/csrc/acn_qp_vjp_long.hpp: gradients through the solve at horizons 33 ... 288, N <= 64,
behind ``acnqp_set_long_vjp`` / ``SiteHandle(..., vjp_long=True)``) against the numpy specification tests/vjp_spec.py with its
row table raised to the worst case of the shape, problem by problem on the pools of tests/polish_long_cases.py
(tests/test_vjp_long_spec.py proves them fit on the CPU), and the layers above it.

As in tests/test_vjp_gpu.py the point (x, y) fed to the entry is the polish specification's own certified one: kernel and
specification take the same working set and differ by the order of their sums and by the way they solve the same
regularised system.

KERNEL_TOL_LONG: |kernel - specification|_inf / max(1, |specification|_inf) per output, ten times the worst measured on the
MI355X over every case of this file (the short file's rule: the two differ by summation order alone).  Measured: gq 1.65e-14,
gcap 6.99e-15, grow 2.44e-15, gub 2.52e-15, res 1.56e-14 (all ct54_t48_peak[0]: 527 free variables against a peak row), glb
2.02e-15 (b52_t144[0]: 874 rows); "reproduce" (tests.test_vjp_gpu.compare: where the tight rows are dependent, H a + C'm = g)
9.39e-11 (n8_t144[3]: 568 rows of rank 129, where reg = 1e-9 pd weighs in).  A difference above 1e-6 on a full-rank problem
would be a bug, not a tolerance.  solve_qp at ct54_t48 (eps 1e-9, long polish behind the solve): all six end SOLVED, with
stationarity res[1] between 1.5e-12 and 5.1e-10.
"""
import functools
import types

import numpy as np
import pytest

from adacharge_amd import backend
from tests import helpers as H
from tests import polish_cases as PC
from tests import polish_long_cases as PLC
from tests import test_vjp_gpu as TVG
from tests import vjp_spec as VS
from tests.test_vjp_gpu import device_vjp, pad_ref
from tests.test_vjp_long_spec import long_points, long_ref, long_weights

pytestmark = pytest.mark.gpu

KERNEL_TOL_LONG = dict(gq=1.65e-13, gcap=6.99e-14, grow=2.44e-14, glb=2.02e-14, gub=2.52e-14, res=1.56e-13, reproduce=9.39e-10)
ALL_ROWS = 48 * 288   # the row tables of the long kernels at their largest shape: the specification gives nothing up for `rows`

# (pool, t_max, K): None is the pool's own
CASES = (("ct54_t48", None, None), ("ct54_t48", 49, None), ("ct54_t48", None, 4), ("ct54_t48_peak", None, None),
         ("ct54_lin_multi", None, None), ("b52_t48_two", None, None), ("n64_lin_t96_peak", None, None), ("n8_t144", None, None),
         ("n8_t288", 288, None), ("b52_t144", None, None))


@functools.lru_cache(maxsize=None)
def handle(name, polish_long=False):
    return backend.SiteHandle(PLC.pool(name).site, 0, polish_long=polish_long, vjp_long=True)


@pytest.fixture
def compare(monkeypatch):
    """tests.test_vjp_gpu.compare, held to KERNEL_TOL_LONG and with the specification's row table raised where it asks the
    specification what a kernel's answer reproduces (dependent rows)"""
    monkeypatch.setattr(TVG, "KERNEL_TOL", KERNEL_TOL_LONG)
    monkeypatch.setattr(TVG, "VS", types.SimpleNamespace(OUTPUTS=VS.OUTPUTS, vjp=functools.partial(VS.vjp, max_rows=ALL_ROWS)))
    return TVG.compare


def padded(name, t_max, k):
    """a pool's problems, certified points and weights at a padded shape"""
    batch, x, y, status = long_points(name)
    t_max, k = t_max or batch.Tm, k or batch.K
    g = long_weights(x.shape)
    return H.pad_batch(batch, t_max, k), H.pad_result(x, t_max), H.pad_result(y, t_max), H.pad_result(g, t_max), status.copy(), t_max, k


@pytest.mark.parametrize("name,t_max,k", CASES, ids=lambda v: str(v))
def test_kernel_matches_specification_problem_by_problem(name, t_max, k, compare):
    pb, x, y, g, status, t_max, k = padded(name, t_max, k)
    assert 33 <= t_max <= 288
    got = device_vjp(handle(name), pb, x, y, g, status)
    ref, each = long_ref(name)
    for b in range(pb.B):
        compare(f"{name} {t_max}x{k} [{b}]", got, pad_ref(each[b], t_max, k), b, (pb.subset(slice(b, b + 1)), x[b], y[b], g[b]))
    assert (got["info"][status == 1, 0] == VS.DONE).all()
    for b in np.flatnonzero(status != 1):   # (n64_lin_t96_peak[3]: infeasible, enters as MAX_ITER)
        assert got["info"][b].tolist() == [VS.BAD_STATUS, 0, 0, 0]
        assert all((got[n][b] == 0).all() and not np.signbit(got[n][b]).any() for n in VS.OUTPUTS)
    if name == "n64_lin_t96_peak":
        assert status[3] == backend.STATUS_MAX_ITER
    if name == "n8_t144":
        assert pb.Tm == 139 and all(e["rank"] < e["rows_c"] for e in each) and (ref["info"][:, 1] > 256).sum() == 3 and ref["info"][:, 1].max() == 568
    if name == "n8_t288":
        assert pb.Tm == 288 and (np.abs(got["gq"][:, :, 256:]).max() > 0)   # a period index at or above 256 carries a gradient


def test_slab_reuse_and_position():
    """more problems than workgroups: every workgroup takes several in turn in its one slab, and every copy of a problem gets
    the bits it gets in a launch of the pool's own four"""
    import torch

    pb, x, y, g, status, _, _ = padded("n8_t144", None, None)
    h = handle("n8_t144")
    own = device_vjp(h, pb, x, y, g, status)
    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    order = np.random.default_rng(3).permutation(np.arange(n) % pb.B)
    many = device_vjp(h, pb.subset(order), x[order], y[order], g[order], status[order])
    assert (own["info"][:, 0] == VS.DONE).all() and np.abs(own["gq"]).max() > 0
    for name in VS.OUTPUTS + ("info",):
        assert np.array_equal(many[name], own[name][order]), name


def test_host_entry_gives_the_device_entrys_bits():
    pb, x, y, g, status, _, _ = padded("ct54_lin_multi", None, None)
    h = handle("ct54_lin_multi")
    dev = device_vjp(h, pb, x, y, g, status)
    zeros = np.zeros(pb.B)
    v = h.vjp(pb, backend.BatchResult(x, status, status, zeros, zeros, zeros, y=y), g)
    for name, a in (("gq", v.q), ("gcap", v.cap), ("grow", v.rows), ("glb", v.lb), ("gub", v.ub), ("res", v.res), ("info", v.info)):
        assert np.array_equal(a, dev[name]), name
    assert (dev["info"][:, 0] == VS.DONE).all()


def test_the_switch():
    import torch

    from adacharge_amd.acn import InfrastructureInfo
    from adacharge_amd.builder import make_site

    batch, x, y, g = TVG.linear_seven()
    infra, _ = H.caltech_interface()

    def attempt(h, b, match, mg=None):
        dev = backend.DeviceBatch(b, "cuda:0", want_y=True)
        if mg is not None:   # (a handle whose site has other rows: y of its shape)
            dev.y = torch.zeros((b.B, mg, b.Tm), dtype=torch.float64, device="cuda:0")
        B, N, Tm, K = b.B, b.N, b.Tm, b.K
        nrow = h.site.M + int(bool(h.site.has_peak))
        new = lambda *s: torch.full(s, 123.0, dtype=torch.float64, device="cuda:0")
        outs = [new(B, N, Tm), new(B, K, N), new(B, nrow, Tm), new(B, 2), new(B, N, Tm), new(B, N, Tm)]
        info = torch.full((B, 4), -7, dtype=torch.int32, device="cuda:0")
        with pytest.raises(ValueError, match=match):
            h.vjp_device(dev, new(B, N, Tm), outs[0], outs[1], outs[2], info, outs[3], glb=outs[4], gub=outs[5],
                         stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert all(bool((o == 123.0).all()) for o in outs) and bool((info == -7).all()), match

    # off: the refusal as it was
    attempt(TVG.handle(("golden", 0)), H.pad_batch(batch, 33, 1), r"t_max is 33, horizons 1 \.\.\. 32 are served")
    # on, at a horizon the short kernel serves: the same kernel, the same bits
    for cone in (0, 1):
        on = backend.SiteHandle(TVG.handle(("golden", cone)).site, 0, vjp_long=True)
        for key in TVG.GOLDEN:
            gb, gx_, gy, gg, _ = TVG.golden_ref(key)
            if int(gb.site.cone) != cone:
                continue
            pb = H.pad_batch(gb, 12, 1)
            args = (pb, H.pad_result(gx_[None], 12), H.pad_result(gy[None], 12), H.pad_result(gg[None], 12))
            a, b_ = device_vjp(TVG.handle(("golden", cone)), *args), device_vjp(on, *args)
            for name in VS.OUTPUTS + ("info",):
                assert np.array_equal(a[name], b_[name], equal_nan=False), (key, name)
            assert a["info"][0, 0] == VS.DONE
        if cone == 0:   # on: the new refusals, outputs untouched
            attempt(on, H.pad_batch(batch, 289, 1), r"t_max is 289, horizons 1 \.\.\. 288 are served")
        on.close()
    n = batch.N
    bare = InfrastructureInfo(np.zeros((0, 0)), np.zeros(0), np.zeros(n), np.full(n, 208.0), max_pilot=np.full(n, 32.0), min_pilot=np.full(n, 8.0))
    hb = backend.SiteHandle(make_site(bare, "LINEAR"), 0, vjp_long=True)
    assert hb.site.Mg == 0
    attempt(hb, H.pad_batch(batch, 40, 1), "t_max is 40 and the site has no row", mg=0)
    hb.close()
    wide = PC.site_pool((72, 4, 0.4), "LINEAR", (12,), 2, 77)
    hw = backend.SiteHandle(wide.site, 0, vjp_long=True)
    attempt(hw, H.pad_batch(wide, 40, 2), "72 EVSEs")
    hw.close()
    flat = make_site(infra, "LINEAR", with_flat=True)
    hf = backend.SiteHandle(flat, 0, vjp_long=True)
    attempt(hf, H.pad_batch(batch, 40, 1), "load-flattening or demand-charge row", mg=flat.Mg)
    hf.close()


def test_solve_qp_backward_at_horizon_48_is_the_specification_at_the_devices_answer(compare):
    """end to end on ct54_t48 at eps 1e-9 with the long polish behind the solve: for every problem that ends SOLVED the
    gradients are the specification's at the device's OWN (x, y), within the tolerances of the kernel test.
    Stationarity res[1] of the device's answers, measured on the MI355X: 1.5e-12 ... 5.1e-10, all six SOLVED (printed)."""
    import torch

    from adacharge_amd import diff, solve_qp

    name = "ct54_t48"
    batch = PLC.pool(name)
    h = handle(name, polish_long=True)
    w = np.random.default_rng(9).standard_normal((batch.B, batch.N, batch.Tm))
    opts = backend.default_options(eps_abs=1e-9, eps_rel=1e-9)
    tmpl = backend.DeviceBatch(batch, "cuda:0", want_y=True)
    q, cap, lb, ub = (getattr(tmpl, k).clone().requires_grad_(True) for k in ("q", "s_cap", "lb", "ub"))
    x = solve_qp(h, tmpl, q, cap, lb, ub, options=opts)
    (torch.from_numpy(w).to("cuda:0") * x).sum().backward()
    bad = diff.check_last_backward()
    # the same solve by hand: the same bits, and its multipliers
    h.solve_device(tmpl, opts, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(tmpl.x, x.detach())
    xs, ys, st = tmpl.x.cpu().numpy(), tmpl.y.cpu().numpy(), tmpl.status.cpu().numpy()
    solved = np.flatnonzero(st == 1)
    print(f"[vjp-long] solve_qp {name}: status {st.tolist()}")
    assert len(solved) >= 4, st
    assert bad == int((~np.isin(st, (1, 5))).sum())   # no SOLVED problem without a gradient
    direct = device_vjp(h, batch, xs, ys, w, st)
    print(f"[vjp-long] solve_qp {name}: stationarity res[1] {direct['res'][:, 1].tolist()}")
    for nm, t in (("gq", q), ("gcap", cap), ("glb", lb), ("gub", ub)):
        assert np.array_equal(t.grad.cpu().numpy(), direct[nm]), nm
    for b in solved:
        one = batch.subset(slice(b, b + 1))
        ref = VS.vjp(one, 0, xs[b], ys[b], w[b], int(st[b]), max_rows=PLC.worst_rows(batch.site, batch.Tm))
        assert direct["info"][b, 0] == VS.DONE
        compare(f"solve_qp {name}[{b}]", direct, ref, b, (one, xs[b], ys[b], w[b]))


def test_schedule_gradients_at_horizon_48():
    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, quick_charge, sites, total_energy
    from adacharge_amd.acn import Interface

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3), ObjectiveComponent(total_energy, 0.5)]
    sl = sites.random_sessions_general(infra, 48, np.random.default_rng(75), two_per_evse=False)
    aco = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC", solver_options={"vjp_long": True})
    rates = aco.solve(sl, infra)
    N, T = rates.shape
    assert T > 32 and aco.last_batch.Tm == T
    w = np.random.default_rng(4).standard_normal((N, T))
    sg = aco.schedule_gradients(w)
    assert set(sg) == {"q", "energy_demands", "infrastructure_limits", "rate_bounds", "info"}
    assert set(sg["energy_demands"]) == {s.session_id for s in sl} and set(sg["infrastructure_limits"]) == set(infra.constraint_ids)
    batch, res = aco.last_batch, aco.last_result
    gx = H.pad_result(w[None], batch.Tm)
    v = res.handle.vjp(batch, res, gx, options=aco._last_options)
    assert res.handle.vjp_long and sg["info"]["verdict"] == 0 and sg["info"]["free"] == v.info[0, 3] > 0
    assert np.array_equal(sg["q"], v.q[0][:, :T]) and sg["q"].shape == (N, T)
    assert np.array_equal(sg["rate_bounds"]["lb"], v.lb[0][:, :T]) and np.array_equal(sg["rate_bounds"]["ub"], v.ub[0][:, :T])
    for s in sl:
        i = infra.get_station_index(s.station_id)
        k_i = infra.voltages[i] * iface.period / 1e3 / 60
        slot = int(np.flatnonzero((batch.s_len[0, :, i] > 0) & (batch.s_off[0, :, i] == s.arrival_offset))[0])
        assert sg["energy_demands"][s.session_id] == v.cap[0, slot, i] / k_i
    for j, cid in enumerate(infra.constraint_ids):
        assert sg["infrastructure_limits"][cid] == v.rows[0, j].sum()
    assert any(sg["energy_demands"].values())
    # without the option: refused as before
    plain = AdaptiveChargingOptimization(obj, iface, constraint_type="SOC")
    plain.solve(sl, infra)
    with pytest.raises(ValueError, match=r"horizons 1 \.\.\. 32 are served"):
        plain.schedule_gradients(w)
