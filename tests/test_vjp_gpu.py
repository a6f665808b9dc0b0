"""The adjoint KKT kernel (acnqp_vjp_device / acnqp_vjp_host, adacharge_amd/csrc/acn_qp_vjp.hpp) against its numpy
specification (tests/vjp_spec.py), and the layers above it (SiteHandle.vjp, schedule_gradients, solve_qp).

The point (x, y) fed to the entry is the polish specification's own certified one, so the solver's accuracy is not in the
comparison: kernel and specification take the same working set and differ by the order of their sums and by the way they
solve the same regularised system (per-period blocks and a capacitance matrix against one dense solve).
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from adacharge_amd import backend
from tests import helpers as H
from tests import polish_cases as PC
from tests import vjp_spec as VS
from tests.test_vjp_spec import certified, weights

pytestmark = pytest.mark.gpu

GOLDEN = ("c00", "c01", "c05", "c09", "c06", "c07")
LINEAR = ("c00", "c01", "c05", "c09")
SHAPES = ((12, 1), (13, 1), (17, 1), (32, 1), (12, 2), (12, 4))   # (t_max, k_sessions): both instantiations, TQ = 3, 4, 5, 8
# |kernel - specification|_inf / max(1, |specification|_inf) per output: ten times the worst measured on the MI355X over every
# case of this file (the six golden cases at the six shapes, the four pools, solve_qp's seven problems).  Measured: gq 5.2e-15
# (peak[3]), gcap 4.2e-15 (peak[3]), grow 3.0e-15 (eq[7]), glb 1.2e-15 (eq[7]), gub 9.6e-16 (peak[6]), res 4.8e-15 (eq[7]):
# the kernel and numpy solve the same system in another order and differ by rounding alone.  (A difference above 1e-6 would
# be a bug, not a tolerance.)  "reproduce": see compare(); worst 1.8e-11 (n8[1]), where reg = 1e-9 pd weighs in.
KERNEL_TOL = dict(gq=5.2e-14, gcap=4.2e-14, grow=3.0e-14, glb=1.2e-14, gub=9.6e-15, res=4.8e-14, reproduce=1.8e-10)
POOLS = {"peak": "ct54_soc_t24_peak", "eq": "ct54_lin_eq_peak", "n64": "n64_lin_t16_peak", "n8": "n8_soc"}


@functools.lru_cache(maxsize=None)
def handle(site_key):
    """one handle per site: ("golden", cone) or a pool's name"""
    site = certified("c06" if site_key[1] else "c01")[0].site if site_key[0] == "golden" else PC.pool(site_key[1]).site
    return backend.SiteHandle(site, 0)


def stack(batches):
    """batches of one site and one padded shape as one batch"""
    out = copy.copy(batches[0])
    for name in out._PER_PROBLEM:
        parts = [getattr(b, name) for b in batches]
        setattr(out, name, None if parts[0] is None else np.concatenate(parts))
    out.B = len(out.T)
    return out


def device_vjp(h, batch, x, y, g, status=None, bounds=True, poison=float("nan")):
    """acnqp_vjp_device with every output poisoned; host arrays back: dict of VS.OUTPUTS and info"""
    import torch

    dev = backend.DeviceBatch(batch, "cuda:0", want_y=True)
    dev.x.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    dev.y.copy_(torch.from_numpy(np.ascontiguousarray(y)))
    dev.status.copy_(torch.from_numpy(np.ones(batch.B, np.int32) if status is None else np.ascontiguousarray(status, np.int32)))
    B, N, Tm, K = batch.B, batch.N, batch.Tm, batch.K
    nrow = batch.site.M + int(bool(batch.site.has_peak))
    new = lambda *s: torch.full(s, poison, dtype=torch.float64, device="cuda:0")
    out = dict(gq=new(B, N, Tm), gcap=new(B, K, N), grow=new(B, nrow, Tm), glb=new(B, N, Tm) if bounds else None,
               gub=new(B, N, Tm) if bounds else None, res=new(B, 2))
    info = torch.full((B, 4), -7, dtype=torch.int32, device="cuda:0")
    h.vjp_device(dev, torch.from_numpy(np.ascontiguousarray(g)).to("cuda:0"), out["gq"], out["gcap"], out["grow"], info, out["res"],
                 glb=out["glb"], gub=out["gub"], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    got["info"] = info.cpu().numpy()
    return got


def pad_ref(ref, t_max, k):
    """the specification's outputs at a padded shape: zeros in the padding"""
    out = {}
    for name, a in ref.items():
        if name == "gcap":
            out[name] = np.zeros((k, a.shape[1]))
            out[name][: a.shape[0]] = a
        elif name in ("gq", "glb", "gub", "grow"):
            out[name] = H.pad_result(a[None], t_max)[0]
        else:
            out[name] = a
    return out


def compare(tag, got, ref, b, point=None):
    """per output |kernel - specification|_inf / max(1, |specification|_inf), printed, then held to KERNEL_TOL; info is equal.
    Where the specification finds DEPENDENT tight rows (rank of C below its rows: c00) the multipliers m are one of many and
    the regularised solve fixes the least-norm one only to rounding / reg -- numpy's dense and block-wise solves of that
    system differ by 1.1e-5 there, the kernel by 1.7e-6: gq, the residuals and the counts are held as everywhere, gcap, grow,
    glb and gub to their zeros and to reproducing g (``point`` = (batch, x, y, g): H a + C'm = g within KERNEL_TOL["reproduce"])."""
    worst = {}
    dependent = ref["rank"] < ref["rows_c"]
    for name in VS.OUTPUTS:
        k, s = (got[name] if b is None else got[name][b]), ref[name]
        assert k.shape == s.shape, (tag, name, k.shape, s.shape)
        assert np.isfinite(k).all(), (tag, name, "an output element was not written")
        worst[name] = float(np.abs(k - s).max() / max(1.0, np.abs(s).max())) if s.size else 0.0
        if name != "res":
            assert ((k == 0) | (s != 0)).all(), (tag, name, "non-zero where the specification has an exact zero")
    if dependent:
        batch, x, y, g = point
        mine = VS.vjp(batch, 0, x, y, g, given={k: got[k][b] for k in ("gq", "gcap", "grow")})["given_res"]
        print(f"[vjp] {tag}: dependent rows: " + " ".join(f"({n} {worst.pop(n):.2e})" for n in ("gcap", "grow", "glb", "gub")) + f" reproduces g to {mine:.2e}")
        worst["reproduce"] = mine
    print(f"[vjp] {tag}: " + " ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    info = got["info"] if b is None else got["info"][b]
    assert info.tolist() == ref["info"].tolist(), (tag, info, ref["info"])
    assert all(v <= KERNEL_TOL[n] for n, v in worst.items()), (tag, worst)
    return worst


@functools.lru_cache(maxsize=None)
def golden_ref(key):
    batch, x, y = certified(key)
    g = weights(batch, 23)
    return batch, x, y, g, VS.vjp(batch, 0, x, y, g)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"T{s[0]}K{s[1]}")
@pytest.mark.parametrize("key", GOLDEN)
def test_kernel_matches_specification_on_the_golden_cases(key, shape):
    batch, x, y, g, ref = golden_ref(key)
    t_max, k = shape
    assert ref["info"][0] == VS.DONE and ref["info"][1] > 0 and ref["info"][3] > 0
    pb = H.pad_batch(batch, t_max, k)
    got = device_vjp(handle(("golden", int(batch.site.cone))), pb, H.pad_result(x[None], t_max), H.pad_result(y[None], t_max),
                     H.pad_result(g[None], t_max))
    compare(f"{key} {t_max}x{k}", got, pad_ref(ref, t_max, k), 0,
            (pb, H.pad_result(x[None], t_max)[0], H.pad_result(y[None], t_max)[0], H.pad_result(g[None], t_max)[0]))


@functools.lru_cache(maxsize=None)
def pool_points(name):
    """the first eight problems of a pool with the polish specification's certified point from the twin's answer; status 2
    where there is none (an infeasible problem, a polish that gives up)"""
    full = PC.pool(name)
    batch = full.subset(slice(0, 8))
    sol = PC.twin(name)
    todo = [b for b in range(8) if sol["status"][b] in (1, 5)]
    res = PC.spec_many([PC.spec_args(batch, b, sol["x"][b], sol["y"][b]) for b in todo])
    x, y = np.zeros((8, batch.N, batch.Tm)), np.zeros((8, batch.site.Mg, batch.Tm))
    status = np.full(8, backend.STATUS_MAX_ITER, np.int32)
    for b, (xb, info) in zip(todo, res):
        if info["ok"]:
            T = xb.shape[1]
            x[b, :, :T], y[b, :, :T], status[b] = xb, info["y"], 1
    return batch, x, y, status


@pytest.mark.parametrize("which", list(POOLS))
def test_kernel_matches_specification_on_the_pools(which):
    """a peak row with discs at horizon 24 (vjp_kernel<8>), equality rows with a peak, N = 64 (all 256 threads own
    variables), a site of 8 EVSEs; K = 2 and horizons below t_max in the first three"""
    batch, x, y, status = pool_points(POOLS[which])
    assert (status == 1).sum() >= 5, status
    if which == "eq":
        assert batch.s_eq.all() and batch.site.has_peak
    if which == "n64":
        assert batch.N == 64
    g = np.random.default_rng(5).standard_normal(x.shape)
    got = device_vjp(handle(("pool", POOLS[which])), batch, x, y, g, status)
    ref, each = VS.vjp_batch(batch, x, y, g, status)
    for b in range(batch.B):
        compare(f"{which}[{b}]", got, each[b], b, (batch.subset(slice(b, b + 1)), x[b], y[b], g[b]))
    assert (ref["info"][status == 1, 0] == VS.DONE).all() and (got["info"][status != 1, 0] == VS.BAD_STATUS).all()


@functools.lru_cache(maxsize=None)
def linear_seven():
    """seven LINEAR golden problems in one batch: c00 c01 c05 c09 c00 c01 c05"""
    keys = LINEAR + LINEAR[:3]
    parts = [certified(k) for k in keys]
    batch = stack([p[0] for p in parts])
    x, y = np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts])
    return batch, x, y, np.random.default_rng(9).standard_normal(x.shape)


def test_host_entry_gives_the_device_entrys_bits(monkeypatch):
    batch, x, y, g = linear_seven()
    h = handle(("golden", 0))
    status = np.ones(7, np.int32)
    dev = device_vjp(h, batch, x, y, g, status)
    point = backend.BatchResult(x, status, status, np.zeros(7), np.zeros(7), np.zeros(7), y=y)
    for chunk in (None, "3"):   # one chunk, and chunks of 3, 3, 1
        if chunk:
            monkeypatch.setenv("ACNQP_POST_CHUNK", chunk)
        v = h.vjp(batch, point, g)
        for name, a in (("gq", v.q), ("gcap", v.cap), ("grow", v.rows), ("glb", v.lb), ("gub", v.ub), ("res", v.res), ("info", v.info)):
            assert np.array_equal(a, dev[name]), (chunk, name)
    nb = h.vjp(batch, point, g, want_bounds=False)
    assert nb.lb is None and nb.ub is None and np.array_equal(nb.q, dev["gq"])


def test_same_bits_alone_and_at_position_6_of_7():
    batch, x, y, g = linear_seven()
    h = handle(("golden", 0))
    seven = device_vjp(h, batch, x, y, g)
    one = slice(6, 7)
    alone = device_vjp(h, batch.subset(one), x[one], y[one], g[one])
    for name in VS.OUTPUTS + ("info",):
        assert np.array_equal(alone[name][0], seven[name][6]), name
    assert np.abs(seven["gq"][6]).max() > 0


def test_unsolved_problem_gets_zeros_and_verdict_1():
    batch, x, y, g = linear_seven()
    status = np.ones(7, np.int32)
    status[3] = backend.STATUS_MAX_ITER
    got = device_vjp(handle(("golden", 0)), batch, x, y, g, status)
    assert got["info"][3].tolist() == [VS.BAD_STATUS, 0, 0, 0]
    assert all((got[k][3] == 0).all() and not np.signbit(got[k][3]).any() for k in VS.OUTPUTS)
    assert (got["info"][[0, 1, 2, 4, 5, 6], 0] == VS.DONE).all() and np.abs(got["gq"][2]).max() > 0


def test_every_refusal_leaves_the_outputs_untouched():
    """ACNQP_ERR_INVALID (ValueError in the binding) with the reason, before any device work"""
    import torch

    from adacharge_amd.builder import make_site

    batch, x, y, g = linear_seven()
    infra, _ = H.caltech_interface()
    wide = PC.site_pool((72, 4, 0.4), "LINEAR", (12,), 2, 77)

    def attempt(h, b, match, alias=False, mg=None):
        dev = backend.DeviceBatch(b, "cuda:0", want_y=True)
        if mg is not None:   # (a handle whose site has another row: y of its shape)
            dev.y = torch.zeros((b.B, mg, b.Tm), dtype=torch.float64, device="cuda:0")
        B, N, Tm, K = b.B, b.N, b.Tm, b.K
        nrow = h.site.M + int(bool(h.site.has_peak))
        new = lambda *s: torch.full(s, 123.0, dtype=torch.float64, device="cuda:0")
        outs = [new(B, N, Tm), new(B, K, N), new(B, nrow, Tm), new(B, 2), new(B, N, Tm), new(B, N, Tm)]
        info = torch.full((B, 4), -7, dtype=torch.int32, device="cuda:0")
        gx = outs[0] if alias else new(B, N, Tm)
        with pytest.raises(ValueError, match=match):
            h.vjp_device(dev, gx, outs[0], outs[1], outs[2], info, outs[3], glb=outs[4], gub=outs[5],
                         stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert all(bool((o == 123.0).all()) for o in outs) and bool((info == -7).all()), match

    h = handle(("golden", 0))
    attempt(h, H.pad_batch(batch, 33, 1), "t_max is 33")
    attempt(h, H.pad_batch(batch, 12, 5), "k_sessions is 5")
    attempt(h, batch, "gq overlaps gx", alias=True)
    hw = backend.SiteHandle(wide.site, 0)
    attempt(hw, wide, "72 EVSEs")
    hw.close()
    for kw in (dict(with_flat=True), dict(with_max=True)):
        site = make_site(infra, "LINEAR", **kw)
        hf = backend.SiteHandle(site, 0)
        attempt(hf, batch, "load-flattening or demand-charge row", mg=site.Mg)
        hf.close()
    # a foreign shape: the problems say nothing of the peak row the handle's site has
    peak_site = make_site(infra, "LINEAR", with_peak=True)
    hp = backend.SiteHandle(peak_site, 0)
    attempt(hp, batch, "peak is null", mg=peak_site.Mg)
    hp.close()
    lib = backend.load_library()
    poison = torch.full((7, 4), -7, dtype=torch.int32, device="cuda:0")
    assert lib.acnqp_vjp_device(None, *[None] * 11, C.c_void_p(poison.data_ptr()), None, None) == -1
    assert b"null handle" in lib.acnqp_last_error()
    torch.cuda.synchronize()
    assert bool((poison == -7).all())


def test_solve_qp_backward_is_the_specification_at_the_devices_answer():
    """end to end: strictly convex 54 x 12 problems at eps 1e-9, loss sum(w x): q.grad is the specification's gq at the
    device's OWN (x, y), for the problems whose stationarity res[1] is below 1e-8; the other gradients are the kernel's"""
    import torch

    from adacharge_amd import solve_qp
    from adacharge_amd import diff

    batch, _, _, w = linear_seven()
    assert (batch.pdiag > 0).all()
    h = handle(("golden", 0))
    opts = backend.default_options(eps_abs=1e-9, eps_rel=1e-9)
    tmpl = backend.DeviceBatch(batch, "cuda:0", want_y=True)
    q, cap, lb, ub = (getattr(tmpl, k).clone().requires_grad_(True) for k in ("q", "s_cap", "lb", "ub"))
    x = solve_qp(h, tmpl, q, cap, lb, ub, options=opts)
    wt = torch.from_numpy(w).to("cuda:0")
    (wt * x).sum().backward()
    assert diff.check_last_backward() == 0
    # the same solve by hand: the same bits, and its multipliers
    h.solve_device(tmpl, opts, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(tmpl.x, x.detach())
    xs, ys, st = tmpl.x.cpu().numpy(), tmpl.y.cpu().numpy(), tmpl.status.cpu().numpy()
    direct = device_vjp(h, batch, xs, ys, w, st)
    for name, t in (("gq", q), ("gcap", cap), ("glb", lb), ("gub", ub)):
        assert np.array_equal(t.grad.cpu().numpy(), direct[name]), name
    ref, _ = VS.vjp_batch(batch, xs, ys, w, st)
    held = [b for b in range(batch.B) if direct["res"][b, 1] < 1e-8]
    print(f"[vjp] solve_qp: stationarity {direct['res'][:, 1]}, held {held}")
    assert len(held) >= 4, direct["res"]
    for b in held:
        err = float(np.abs(direct["gq"][b] - ref["gq"][b]).max() / max(1.0, np.abs(ref["gq"][b]).max()))
        print(f"[vjp] solve_qp[{b}]: |q.grad - specification| {err:.2e}")
        assert err <= KERNEL_TOL["gq"], (b, err)


def test_schedule_gradients_in_the_references_units():
    from adacharge_amd import AdaptiveChargingOptimization, ObjectiveComponent, equal_share, quick_charge

    g = H.load_golden()
    infra, iface = H.caltech_interface()
    sl, meta, _ = H.golden_case(g, "c06")
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, meta["es"])]
    aco = AdaptiveChargingOptimization(obj, iface, meta["ct"], False)
    rates = aco.solve(sl, infra)
    N, T = rates.shape
    w = np.random.default_rng(4).standard_normal((N, T))
    sg = aco.schedule_gradients(w)
    assert set(sg) == {"q", "energy_demands", "infrastructure_limits", "rate_bounds", "info"}
    assert set(sg["energy_demands"]) == {s.session_id for s in sl} and set(sg["infrastructure_limits"]) == set(infra.constraint_ids)
    batch, res = aco.last_batch, aco.last_result
    gx = H.pad_result(w[None], batch.Tm)
    v = res.handle.vjp(batch, res, gx, options=aco._last_options)
    assert sg["info"]["verdict"] == 0 and sg["info"]["free"] == v.info[0, 3] > 0
    assert np.array_equal(sg["q"], v.q[0][:, :T]) and sg["q"].shape == (N, T)
    assert np.array_equal(sg["rate_bounds"]["lb"], v.lb[0][:, :T]) and np.array_equal(sg["rate_bounds"]["ub"], v.ub[0][:, :T])
    for s in sl:
        i = infra.get_station_index(s.station_id)
        k_i = infra.voltages[i] * iface.period / 1e3 / 60
        slot = int(np.flatnonzero((batch.s_len[0, :, i] > 0) & (batch.s_off[0, :, i] == s.arrival_offset))[0])
        assert sg["energy_demands"][s.session_id] == v.cap[0, slot, i] / k_i
    for j, cid in enumerate(infra.constraint_ids):
        assert sg["infrastructure_limits"][cid] == v.rows[0, j].sum()
    assert any(sg["energy_demands"].values()) and any(sg["infrastructure_limits"].values())
    # ... and they are the specification's at the solver's own answer
    ref = VS.vjp(batch, 0, res.x[0], res.y[0], gx[0], int(res.status[0]))
    print(f"[vjp] schedule_gradients: stationarity {v.res[0, 1]:.2e}")
    if v.res[0, 1] < 1e-8:
        assert np.abs(v.q[0] - ref["gq"]).max() <= KERNEL_TOL["gq"] * max(1.0, np.abs(ref["gq"]).max())
    with pytest.raises(ValueError, match="grad_rates"):
        aco.schedule_gradients(w[:, :1])
