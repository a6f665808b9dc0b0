"""What adacharge_amd/backend.py hands the library: the pointers of ``acnqp_problems`` from a ``DeviceBatch`` and from host
arrays, the pointer rule of the plan classes, the tensor checker -- on CPU tensors, no GPU -- and, on a GPU, that the device
entries give the host entries' bits on a site without and on a site with the load-flattening / demand-charge rows."""
import ctypes as C

import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, backend, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.builder import build_batch, make_site

B, TM = 2, 4


def _small(**site_kw):
    infra = sites.balanced_three_phase(6, pods=1, load_fraction=0.35)
    site = make_site(infra, "SOC", **site_kw)
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
    peaks = [40.0] * B if site.has_peak else None
    return site, build_batch(sites.snapshot_batch(infra, TM, B, seed=3), infra, iface, obj, "SOC", peak_limits=peaks, site=site)


def _addr(field):
    return field or 0   # a NULL c_void_p field reads back as None


def test_device_batch_to_problems():
    import torch

    site, _ = _small()
    dev = backend.DeviceBatch.empty(site, B, TM, 1, "cpu", want_y=True)
    p = backend._device_problems(dev)
    assert (p.batch, p.t_max, p.k_sessions) == (B, TM, 1)
    assert dev.peak is None and p.peak is None and p.warm_x is None and p.warm_y is None
    for k in backend._PROBLEM_ARRAYS:
        if k != "peak":
            assert _addr(getattr(p, k)) == getattr(dev, k).data_ptr() != 0, k
    assert len({getattr(p, k) for k in backend._PROBLEM_ARRAYS}) == len(backend._PROBLEM_ARRAYS)   # no tensor twice
    wx, wy = torch.zeros((B, site.N, TM), dtype=torch.float64), torch.zeros((B, site.Mg, TM), dtype=torch.float64)
    p = backend._device_problems(dev, wx, wy)
    assert (p.warm_x, p.warm_y) == (wx.data_ptr(), wy.data_ptr())
    with_peak = backend.DeviceBatch.empty(site, B, TM, 1, "cpu", with_peak=True)
    assert backend._device_problems(with_peak).peak == with_peak.peak.data_ptr()
    # the tensors have the ABI's dtypes and DeviceBatch(batch) holds the same fields as DeviceBatch.empty
    _, batch = _small()
    full = backend.DeviceBatch(batch, "cpu")
    for k, dt in {**backend._PROBLEM_ARRAYS, **backend._RESULT_ARRAYS}.items():
        for d in (dev, full):
            assert getattr(d, k) is None and k == "peak" or getattr(d, k).dtype == getattr(torch, np.dtype(dt).name), k
        assert k == "peak" or getattr(dev, k).shape == getattr(full, k).shape, k
    assert full.y is None and dev.y.shape == (B, site.Mg, TM)
    assert (dev.horizon == 1).all() and np.array_equal(full.horizon.numpy(), batch.T) and np.array_equal(full.s_cap.numpy(), batch.s_cap)


def test_host_marshaller():
    site, batch = _small()
    assert not site.has_flat and not site.has_max and not site.has_peak
    p, r, res, keep = backend._marshal_batch(site, batch, False, want_y=True)
    assert (p.batch, p.t_max, p.k_sessions) == (B, TM, batch.K)
    assert p.lf is None and p.dc is None and p.dfloor is None and p.peak is None and p.warm_x is None and p.warm_y is None
    for k in ("lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap", "s_eq"):   # already C-contiguous with the ABI's dtype: no copy
        a = getattr(batch, k)
        assert a.flags.c_contiguous and a.dtype == backend._PROBLEM_ARRAYS[k] and getattr(p, k) == a.ctypes.data, k
    assert p.horizon == keep[0]["horizon"].ctypes.data and np.array_equal(keep[0]["horizon"], batch.T)
    for k in backend._RESULT_ARRAYS:
        assert getattr(r, k) == getattr(res, k).ctypes.data and getattr(res, k).dtype == backend._RESULT_ARRAYS[k], k
    assert res.x.shape == (B, site.N, TM) and res.status.shape == (B,) and r.y == res.y.ctypes.data and res.y.shape == (B, site.Mg, TM)
    assert r.x_dev is None
    # an array that is not the ABI's is converted, and the copy is what the struct points to
    batch.q = np.asfortranarray(batch.q)
    batch.s_len = batch.s_len.astype(np.int64)
    p, r, res, keep = backend._marshal_batch(site, batch, False, x_dev=4096)
    assert p.q == keep[0]["q"].ctypes.data != batch.q.ctypes.data and keep[0]["q"].flags.c_contiguous
    assert p.s_len == keep[0]["s_len"].ctypes.data and keep[0]["s_len"].dtype == np.int32
    assert r.y is None and res.y is None and r.x_dev == 4096
    # a site with every optional row passes its arrays
    site, batch = _small(with_peak=True, with_flat=True, with_max=True)
    batch.dc, batch.dfloor = np.ones(B), np.zeros(B)
    p, _, _, keep = backend._marshal_batch(site, batch, False)
    for k in ("peak", "lf", "dc", "dfloor"):
        assert getattr(p, k) == keep[0][k].ctypes.data != 0, k
    # warm starts: shapes are checked
    wx, wy = np.zeros((B, site.N, TM)), np.zeros((B, site.Mg, TM))
    p, _, _, keep = backend._marshal_batch(site, batch, False, warm=(wx, wy))
    assert (p.warm_x, p.warm_y) == (wx.ctypes.data, wy.ctypes.data)
    with pytest.raises(ValueError, match="warm start arrays"):
        backend._marshal_batch(site, batch, False, warm=(wx, wy[:, :-1]))


def test_results_are_reused_when_they_fit():
    first, r = backend._new_results(B, 6, TM, 3, False, True)
    again, r2 = backend._new_results(B, 6, TM, 3, False, False, out=first)
    assert again is first and r2.x == r.x and r.y == first.y.ctypes.data and r2.y is None   # y is handed over only when wanted
    other, _ = backend._new_results(B, 6, TM + 1, 3, False, False, out=first)
    assert other is not first and other.x.shape == (B, 6, TM + 1) and other.y is None
    no_y, _ = backend._new_results(B, 6, TM, 3, False, False)
    assert backend._new_results(B, 6, TM, 3, False, True, out=no_y)[0] is not no_y


def test_problems_by_keyword_and_by_position():
    a = np.zeros(3, np.int32)
    p = backend._Problems(5, 7, 1, s_off=backend._ptr(a))
    assert (p.batch, p.t_max, p.k_sessions, p.s_off) == (5, 7, 1, a.ctypes.data)
    assert all(getattr(p, k) is None for k, _ in backend._Problems._fields_[3:] if k != "s_off")
    q = backend._Problems(5, 7, 1, *[None] * 15)
    assert bytes(q) == bytes(backend._Problems(5, 7, 1))
    assert [k for k, _ in backend._Next._fields_] == [k for k, _ in backend._Problems._fields_[3:] if k != "s_eq"]
    assert backend.SiteHandle._NEXT == tuple(k for k, _ in backend._Next._fields_[:-2])


def test_plan_pointer_rule():
    import torch

    N, A = 6, 3
    seg = np.arange(2 * (B + 1), dtype=np.int32).reshape(2, B + 1)
    table = np.zeros((1, N, TM), np.float32)[:, :, ::2]   # float32 and not contiguous
    plan = backend.AdvancePlan(q_table=table, h_scal=np.zeros((1, 3)), h_row=np.zeros(TM + 1, np.int32), done_tol=0.0, kw_per_amp=0.2,
                               peak_series=np.zeros((B, 0)), a_seg=seg, a_evse=np.zeros(A, np.int32), a_slot=np.zeros(A, np.int32),
                               a_len=np.ones(A, np.int32), a_cap=np.ones(A), a_rate_seg=np.arange(A + 1, dtype=np.int32))
    keep = []
    s = plan._struct(N, 3, 0, 1, keep)
    assert (s.n_evse, s.n_rows, s.n_horizons, s.step, s.peak_len, s.n_arrivals, s.n_rates) == (N, 3, 1, 0, 0, A, 0)
    assert s.a_min is None and s.a_max is None            # None gives NULL
    assert s.peak_series is None                          # an empty array gives NULL
    assert s.a_seg == seg[1].ctypes.data == seg.ctypes.data + 4 * (B + 1)   # row 1 of the 2-D a_seg
    assert plan._struct(N, 3, 0).a_seg == seg.ctypes.data and s.h_scal == plan.h_scal.ctypes.data
    conv = [a for a in keep if a.shape == table.shape]
    assert len(conv) == 1 and conv[0].dtype == np.float64 and conv[0].flags.c_contiguous and s.q_table == conv[0].ctypes.data
    assert np.array_equal(conv[0], table)
    assert any(a is plan.h_scal for a in keep)             # an array that already fits is passed as it is
    assert dict(plan._DTYPES)["a_seg"] == np.int32 and plan._ARRAYS == tuple(k for k, _ in backend._AdvancePlan._fields_[10:])
    none = backend.AdvancePlan(q_table=plan.q_table, h_scal=plan.h_scal, h_row=plan.h_row, done_tol=0.0, kw_per_amp=0.2, a_seg=seg[0])
    assert none._struct(N, 3, 0).a_seg is None             # no arrival: a_seg is NULL whatever is stored
    # tensors give their own address, rows included
    tseg = torch.from_numpy(seg)
    tplan = backend.AdvancePlan(q_table=torch.zeros((1, N, TM), dtype=torch.float64), h_scal=torch.zeros((1, 3), dtype=torch.float64),
                                h_row=torch.zeros(TM + 1, dtype=torch.int32), done_tol=0.0, kw_per_amp=0.2, a_seg=tseg,
                                a_evse=torch.zeros(A, dtype=torch.int32))
    assert tplan._struct(N, 3, 0, 1).a_seg == tseg[1].data_ptr() and tplan._struct(N, 3, 0).q_table == tplan.q_table.data_ptr()
    # PreparePlan: block key_row of a 3-D key
    key = np.zeros((2, B, N), np.int32)
    prep = backend.PreparePlan(key=key, cre=np.zeros((2, N)), cim=np.zeros((2, N)), limits=np.ones(2), min_pilot=np.full(N, 8.0))
    s = prep._struct(N, 1)
    assert (s.n_evse, s.n_infra, s.key, s.min_pilot) == (N, 2, key[1].ctypes.data, prep.min_pilot.ctypes.data)
    assert prep._struct(N).key == key.ctypes.data and prep._struct(N, 1, min_rates=False).min_pilot is None
    assert backend.PreparePlan(key=key[0])._struct(N, 1).key == key.ctypes.data
    # PilotPlan: counts from the arrays, the batch shape from the call
    pil = backend.PilotPlan(backend.PILOTS_DISCRETE, B, TM, N, levels=np.zeros((N, 5)), s_evse=np.zeros(0, np.int32))
    s = pil._struct()
    assert (s.batch, s.t_max, s.n_evse, s.n_infra, s.n_levels, s.n_sessions, s.mode) == (B, TM, N, 0, 5, 0, 1)
    assert s.levels == pil.levels.ctypes.data and s.s_evse is None and s.cre is None and pil._struct(9, 11).batch == 9
    assert pil._ARRAYS == tuple(k for k, _ in backend._PilotPlan._fields_[7:])
    # to_device: every array a tensor of the ABI's dtype, scalars kept
    moved = plan.to_device("cpu")
    assert moved.q_table.dtype == torch.float64 and moved.a_seg.dtype == torch.int32 and moved.a_min is None and moved.kw_per_amp == 0.2
    assert prep.to_device("cpu").key.dtype == torch.int32 and pil.to_device("cpu").mode == backend.PILOTS_DISCRETE


def test_clock_cost_struct_and_tensor_checks():
    import torch

    N, P = 6, 9
    base = dict(q_table=np.zeros((1, N, TM)), h_scal=np.zeros((1, 3)), h_row=np.zeros(TM + 1, np.int32), done_tol=0.0, kw_per_amp=0.2)
    assert backend.AdvancePlan(**base)._cost_struct(N) is None
    with pytest.raises(ValueError, match="needs c_coef, c_weight and c_series"):
        backend.AdvancePlan(**base, c_coef=1.0)._cost_struct(N)
    with pytest.raises(ValueError, match="c_series must have shape"):
        backend.AdvancePlan(**base, c_coef=1.0, c_weight=np.ones(N), c_series=np.ones(P))._cost_struct(N)
    keep = []
    plan = backend.AdvancePlan(**base, c_coef=2.0, c_weight=np.ones(N, np.float32), c_series=np.ones((B, P)))
    c = plan._cost_struct(N, keep)
    assert (c.n_evse, c.series_len, c.coef, c.series) == (N, P, 2.0, plan.c_series.ctypes.data)
    assert c.weight == keep[0].ctypes.data and keep[0].dtype == np.float64
    w, s = torch.ones(N, dtype=torch.float64), torch.ones((B, P), dtype=torch.float64)
    c = backend.AdvancePlan(**base, c_coef=2.0, c_weight=w, c_series=s)._cost_struct(N)
    assert (c.weight, c.series) == (w.data_ptr(), s.data_ptr())
    for bad in (dict(c_weight=w.float()), dict(c_series=torch.ones((P, B), dtype=torch.float64).t())):   # item size, contiguity
        with pytest.raises(ValueError, match="must be a contiguous"):
            backend.AdvancePlan(**{**base, **dict(c_coef=2.0, c_weight=w, c_series=s), **bad})._cost_struct(N)
    # the checker itself: what the older entries ask (no device given) and what the newer ones ask
    cpu = torch.device("cpu")
    x = torch.zeros((B, N, TM), dtype=torch.float64)
    backend._want(None, "x", np.float64, (1,), cpu)
    backend._want(x, "x", np.float64, (B, N, TM))
    backend._want(x, "x", np.float64, None, cpu)
    backend._want(x.view(torch.int64), "x", np.float64, (B, N, TM))     # item size only
    for t, shape, device in ((x, (B, N, TM + 1), None), (x.float(), (B, N, TM), None), (x.transpose(1, 2), (B, TM, N), None),
                             (x.view(torch.int64), None, cpu), (x.numpy(), None, cpu), (x, None, torch.device("meta")),
                             (x[:, :, ::2], None, cpu)):
        with pytest.raises(ValueError, match="x must be a contiguous torch.float64 tensor"):
            backend._want(t, "x", np.float64, shape, device)


def test_call_sites_refuse_before_the_library_is_called():
    """the ValueErrors of ``solve_device``, ``solve_table`` and ``advance_device`` that need no GPU: a handle that was never created"""
    import torch

    site, _ = _small()
    h = backend.SiteHandle.__new__(backend.SiteHandle)
    h.site, h.device, h._h, h._lib = site, 0, None, None
    dev = backend.DeviceBatch.empty(site, B, TM, 1, "cpu", want_y=True)
    wx, wy = torch.zeros((B, site.N, TM), dtype=torch.float64), torch.zeros((B, site.Mg, TM), dtype=torch.float64)
    o = backend.Options()
    with pytest.raises(ValueError, match="go together"):
        h.solve_device(dev, o, warm_x=wx)
    for bad in (dict(warm_x=wx[:1], warm_y=wy), dict(warm_x=wx, warm_y=wy.float()), dict(warm_x=wx.transpose(0, 1), warm_y=wy)):
        with pytest.raises(ValueError, match="must be a contiguous"):
            h.solve_device(dev, o, **bad)
    nxt = backend.DeviceBatch.empty(site, B, TM, 1, "cpu")
    app, flags = torch.zeros((B, site.N), dtype=torch.float64), torch.zeros(B, dtype=torch.int32)
    for bad in (dict(applied=app.float()), dict(applied=app[:, :-1]), dict(flags=flags.long()), dict(flags=flags[:1])):
        with pytest.raises(ValueError, match="must be a contiguous"):
            h.advance_device(**{**dict(cur=dev, nxt=nxt, applied=app, plan=None, step=0, flags=flags), **bad})

    class Plan:
        site, B, N, Tm = h.site, B, 6, TM

    with pytest.raises(ValueError, match="x_dev must be a contiguous"):   # before anything of the plan or of x_dev is read
        h.solve_table(Plan, o, x_dev=wx.float())


def _same_bits_host_and_device(batch):
    import torch

    h = backend.SiteHandle(batch.site, 0)
    host = h.solve(batch, want_y=True)
    hd = h.duals(batch, host)
    dev = backend.DeviceBatch(batch, "cuda:0", want_y=True)
    mu = torch.zeros((batch.B, batch.K, batch.N), dtype=torch.float64, device="cuda:0")
    z, res = torch.zeros_like(dev.x), torch.zeros((batch.B, 4), dtype=torch.float64, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    h.solve_device(dev, stream=stream)
    h.duals_device(dev, mu, res, z=z, stream=stream)
    torch.cuda.synchronize()
    h.close()
    assert np.isin(host.status, backend.ACCEPTED_STATUSES).all(), host.status
    for k in ("x", "status", "iters", "y"):
        assert np.array_equal(getattr(dev, k).cpu().numpy(), getattr(host, k)), k
    assert np.array_equal(mu.cpu().numpy(), hd.mu) and np.array_equal(z.cpu().numpy(), hd.z)
    assert np.array_equal(res.cpu().numpy(), np.stack([hd.stat, hd.energy, hd.site, hd.comp], axis=1))


@pytest.mark.gpu
def test_device_entries_equal_host_entries_without_prox_rows():
    """caltech54, SOC, horizon 12: no flat or max row, so ``solve_device`` / ``duals_device`` hand the library lf, dc and dfloor
    it must not read, where the host entries hand it NULL"""
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]
    batch = build_batch(sites.snapshot_batch(infra, 12, 8, seed=31), infra, iface, obj, "SOC")
    assert not batch.site.has_flat and not batch.site.has_max
    _same_bits_host_and_device(batch)


@pytest.mark.gpu
def test_device_entries_equal_host_entries_with_prox_rows():
    """the same where lf, dc and dfloor are read: load_flattening and demand_charge in one objective"""
    from adacharge_amd import demand_charge, load_flattening, total_energy

    T = 6
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5, "demand_charge": 15.0, "prev_peak": 50.0})
    ext = 40.0 + 30.0 * np.cos(np.arange(T) / T * 2 * np.pi)
    obj = [ObjectiveComponent(load_flattening, 1.0, {"external_signal": ext}), ObjectiveComponent(total_energy, 20.0),
           ObjectiveComponent(demand_charge), ObjectiveComponent(equal_share, 1e-3)]
    batch = build_batch(sites.snapshot_batch(infra, T, 4, seed=32), infra, iface, obj, "SOC")
    assert batch.site.has_flat and batch.site.has_max and batch.lf.all() and batch.dc.all()
    _same_bits_host_and_device(batch)
