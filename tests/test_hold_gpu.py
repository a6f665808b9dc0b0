"""The select and hold kernels (acnqp_select_device / _host, acnqp_hold_device / _host) return the bits of tests/hold_spec.py:
on a 3-EVSE three-phase site and a 65-EVSE one (one wavefront per problem, and four), with and without a peak row, with and
without the flat / max rows (lf, dc, dfloor), and on a site without rows; Tm in {1, 12, 33}, K in {1, 2}, B = 5, m in
{0, 1, 3, 5}, with and without warm_x / warm_y (y).  Float arrays are compared through their int64 bit patterns, so -0.0 and
+inf count.  Every output element is written and nothing beyond the m rows; the inputs are left alone; an out-of-range idx
(S2) and pos (H3) are flagged; the host entries give the device entries' bits at any chunking; every refusal of
include/acn_qp.h returns ACNQP_ERR_INVALID with its message and writes nothing.  No solve: the states are synthetic."""
import ctypes as C
import functools

import numpy as np
import pytest

from adacharge_amd import sites
from tests import hold_spec as spec

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_library")]
B = 5
IDX = {0: [], 1: [4], 3: [0, 2, 4], 5: [0, 1, 2, 3, 4]}
# name: (EVSEs, pods or None for a site without rows, peak, flat, max)
SITES = {"n3": (3, 1, False, False, False), "n3_peak": (3, 1, True, False, False), "n3_flat_max": (3, 1, False, True, True),
         "n3_all": (3, 1, True, True, True), "n65": (65, 4, False, False, False), "n65_all": (65, 4, True, True, True),
         "n3_norows": (3, None, False, False, False), "n65_norows": (65, None, False, False, False)}


@functools.lru_cache(maxsize=None)
def _handle(name):
    from adacharge_amd.acn import InfrastructureInfo
    from adacharge_amd.backend import SiteHandle
    from adacharge_amd.builder import make_site

    n, pods, peak, flat, mx = SITES[name]
    if pods is None:
        infra = InfrastructureInfo(np.zeros((0, 0)), np.zeros(0), np.zeros(n), np.full(n, 208.0), max_pilot=np.full(n, 32.0),
                                   min_pilot=np.full(n, 8.0))
    else:
        infra = sites.balanced_three_phase(n, pods=pods, load_fraction=0.35)
    h = SiteHandle(make_site(infra, "SOC", with_peak=peak, with_flat=flat, with_max=mx), 0)
    assert h.site.N == n and (h.site.Mg == 0) == (pods is None)
    return h


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, keys=None):
    for k in (want if keys is None else keys):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), k


def _fields(site):
    """the arrays of acnqp_problems this site's entries carry"""
    return (("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap", "s_eq") + (("peak",) if site.has_peak else ())
            + (("lf",) if site.has_flat else ()) + (("dc", "dfloor") if site.has_max else ()))


def _state(site, Tm, K, seed):
    """B random problems: finite contents, +inf in peak, -0.0 and exact zeros among the bounds"""
    rng = np.random.default_rng(seed)
    N = site.N
    cur = dict(horizon=rng.integers(1, Tm + 1, B).astype(np.int32), lb=rng.uniform(0, 6, (B, N, Tm)), ub=rng.uniform(8, 32, (B, N, Tm)),
               q=rng.normal(size=(B, N, Tm)), pdiag=rng.uniform(0, 1, B), s_off=rng.integers(0, Tm, (B, K, N)).astype(np.int32),
               s_len=rng.integers(0, Tm + 1, (B, K, N)).astype(np.int32), s_cap=rng.uniform(0, 99, (B, K, N)),
               s_eq=rng.integers(0, 2, B).astype(np.uint8), peak=rng.uniform(40, 90, (B, Tm)), lf=rng.uniform(0, 1, B), dc=rng.uniform(0, 1, B),
               dfloor=rng.uniform(0, 9, B))
    cur["peak"][rng.random((B, Tm)) < 0.3] = np.inf
    cur["peak"][B - 1, 0] = np.inf
    cur["lb"][rng.random((B, N, Tm)) < 0.3] = 0.0
    cur["ub"][rng.random((B, N, Tm)) < 0.2] = 0.0                            # retired windows: lb <= ub does not hold there, and need not
    cur["lb"][0, 0, 0], cur["q"][0, 0, 0] = -0.0, -0.0
    warm_x, warm_y = rng.normal(size=(B, N, Tm)), rng.normal(size=(B, site.Mg, Tm))
    warm_x[B - 1, N - 1, Tm - 1] = -0.0
    return {k: cur[k] for k in _fields(site)}, warm_x, warm_y


def _upload(h, cur, Tm, K, want_y=False):
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = torch.device("cuda", 0)
    st = DeviceBatch.empty(h.site, B, Tm, K, dev, want_y=want_y)
    for k, a in cur.items():
        getattr(st, k).copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    return st


POISON = dict(horizon=-7, s_off=-7, s_len=-7, s_eq=77, status=-7, iters=-7)


def _poisoned(h, Tm, K, want_y=False):
    """a DeviceBatch of B problems whose every array is poisoned: NaN, -7 or 77"""
    import torch
    from adacharge_amd.backend import DeviceBatch, _PROBLEM_ARRAYS

    d = DeviceBatch.empty(h.site, B, Tm, K, torch.device("cuda", 0), want_y=want_y)
    for k in tuple(_PROBLEM_ARRAYS) + ("x", "status", "iters", "y"):
        t = getattr(d, k)
        if t is not None:
            t.fill_(POISON.get(k, float("nan")))
    return d


def _untouched(t, k, rows=slice(None)):
    a = t.cpu().numpy()[rows]
    return bool((a == POISON[k]).all()) if k in POISON else bool(np.isnan(a).all())


def _select_device(h, cur, idx, Tm, K, warm=None):
    import torch
    from adacharge_amd.backend import _PROBLEM_ARRAYS

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st, dense = _upload(h, cur, Tm, K), _poisoned(h, Tm, K)
    m = len(idx)
    didx = up(np.asarray(idx, np.int32)) if m else torch.zeros(0, dtype=torch.int32, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    wx = wy = owx = owy = None
    if warm is not None:
        wx, wy = up(warm[0]), up(warm[1])
        owx, owy = torch.full_like(wx, float("nan")), torch.full_like(wy, float("nan"))
    h.select_device(st, dense, didx, flags, m, warm_x=wx, warm_y=wy, out_warm_x=owx, out_warm_y=owy)
    torch.cuda.synchronize(dev)
    for k, a in cur.items():
        assert np.array_equal(_bits(getattr(st, k).cpu().numpy()), _bits(a)), k              # the state is read only
    out = {k: getattr(dense, k).cpu().numpy()[:m] for k in cur}
    out["flags"] = flags.cpu().numpy()[:m]
    assert (flags.cpu().numpy()[m:] == -7).all()
    for k in _PROBLEM_ARRAYS:                                                               # nothing beyond the m rows, and no array the
        t = getattr(dense, k)                                                               # site has no row for
        if t is not None:
            assert _untouched(t, k, slice(None) if k not in cur else slice(m, None)), k
    if warm is not None:
        assert np.array_equal(_bits(wx.cpu().numpy()), _bits(warm[0])) and np.array_equal(_bits(wy.cpu().numpy()), _bits(warm[1]))
        out["warm_x"], out["warm_y"] = owx.cpu().numpy()[:m], owy.cpu().numpy()[:m]
        assert np.isnan(owx.cpu().numpy()[m:]).all() and np.isnan(owy.cpu().numpy()[m:]).all()
        if h.site.Mg == 0:
            del out["warm_y"]                                                               # (no rows: an array of no elements)
    return out


@pytest.mark.parametrize("Tm", [1, 12, 33])
@pytest.mark.parametrize("name", list(SITES))
def test_select_equals_spec_bit_for_bit(name, Tm, monkeypatch):
    h = _handle(name)
    for K in (1, 2):
        cur, wx, wy = _state(h.site, Tm, K, seed=Tm * 10 + K)
        for m, idx in IDX.items():
            for warm in (None, (wx, wy)):
                want = spec.select(cur, np.asarray(idx, np.int32), *((None, None) if warm is None else warm))
                if h.site.Mg == 0:
                    want.pop("warm_y", None)
                got = _select_device(h, cur, idx, Tm, K, warm)
                _same(got, want)
                assert set(got) == set(want) and not got["flags"].any()
        # S2: an index outside [0, B) gives the empty problem and its flag, whatever stands beside it
        idx = [0, B + 4, B - 1]
        got = _select_device(h, cur, idx, Tm, K, (wx, wy))
        want = spec.select(cur, np.asarray(idx, np.int32), wx, wy)
        if h.site.Mg == 0:
            want.pop("warm_y")
        _same(got, want)
        assert list(got["flags"]) == [0, spec.SELECT_BAD_INDEX, 0] and got["horizon"][1] == 1 and not got["ub"][1].any()
        _same(_select_device(h, cur, [-1], Tm, K), spec.select(cur, np.array([-1], np.int32)))
        # the host entry: the device entry's bits, at any chunking
        for chunk in (None, "2"):
            monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False) if chunk is None else monkeypatch.setenv("ACNQP_POST_CHUNK", chunk)
            for m in (1, 3, 5):
                host = h.select_host(cur, IDX[m], wx, wy if h.site.Mg else None)
                _same(host, _select_device(h, cur, IDX[m], Tm, K, (wx, wy)))
        monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False)
        assert h.select_host(cur, [])["flags"].shape == (0,)


def _hold_case(site, Tm, m, seed):
    rng = np.random.default_rng(seed)
    N, Mg = site.N, site.Mg
    lb, ub = rng.uniform(0, 6, (B, N, Tm)), rng.uniform(8, 32, (B, N, Tm))
    lb[rng.random((B, N, Tm)) < 0.4] = 0.0
    ub[rng.random((B, N, Tm)) < 0.2] = 0.0
    lb[ub == 0.0] = 0.0                                                      # a retired window: lb = ub = 0
    held_x = rng.uniform(-4, 40, (B, N, Tm))                                 # below lb, inside, above ub
    held_x[rng.random((B, N, Tm)) < 0.2] = -0.0
    held_x[rng.random((B, N, Tm)) < 0.1] = 0.0
    held_x[rng.random((B, N, Tm)) < 0.05] = -5e-324                          # the largest negative number: below a zero lb
    ub[0, 0, 0] = np.inf
    held_x[0, 0, 0] = 1e300
    return dict(lb=lb, ub=ub, held_x=held_x, held_y=rng.normal(size=(B, Mg, Tm)), rx=rng.uniform(-1, 33, (m, N, Tm)),
                ry=rng.normal(size=(m, Mg, Tm)), rstatus=rng.choice([1, 2, 3, 5], m).astype(np.int32),
                riters=rng.integers(1, 9000, m).astype(np.int32), prev_status=rng.choice([1, 2, 3, 4, 5], B).astype(np.int32))


def _hold_device(h, c, pos, m, Tm, want_y):
    import torch

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    st = _poisoned(h, Tm, 1, want_y=want_y)
    st.lb.copy_(up(c["lb"]))
    st.ub.copy_(up(c["ub"]))
    dense = _poisoned(h, Tm, 1, want_y=want_y)
    for k, a in (("x", c["rx"]), ("status", c["rstatus"]), ("iters", c["riters"])) + ((("y", c["ry"]),) if want_y else ()):
        getattr(dense, k)[:m].copy_(up(a))
    ins = dict(pos=up(np.asarray(pos, np.int32)), held_x=up(c["held_x"]), held_y=up(c["held_y"]) if want_y else None, prev=up(c["prev_status"]))
    solved = torch.full((B,), 77, dtype=torch.uint8, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    h.hold_device(st, dense.head(m) if m else None, ins["pos"], m, ins["held_x"], ins["prev"], solved, flags, held_y=ins["held_y"])
    torch.cuda.synchronize(dev)
    for t, a in ((st.lb, c["lb"]), (st.ub, c["ub"]), (ins["held_x"], c["held_x"]), (ins["prev"], c["prev_status"]), (dense.x[:m], c["rx"]),
                 (dense.status[:m], c["rstatus"]), (ins["pos"], np.asarray(pos, np.int32))):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))                             # the inputs are read only
    out = dict(x=st.x.cpu().numpy(), status=st.status.cpu().numpy(), iters=st.iters.cpu().numpy(), solved=solved.cpu().numpy(),
               flags=flags.cpu().numpy())
    if want_y:
        out["y"] = st.y.cpu().numpy()
    return out


@pytest.mark.parametrize("Tm", [1, 12, 33])
@pytest.mark.parametrize("name", ["n3", "n3_all", "n65", "n65_all", "n3_norows", "n65_norows"])
def test_hold_equals_spec_bit_for_bit(name, Tm, monkeypatch):
    h = _handle(name)
    for m, idx in IDX.items():
        c = _hold_case(h.site, Tm, m, seed=Tm * 10 + m)
        pos = spec.inverse(idx, B)
        for want_y in (False, True) if h.site.Mg else (False,):
            args = (c["rx"], c["rstatus"], c["riters"], c["held_x"], c["prev_status"], c["lb"], c["ub"])
            want = spec.hold(pos, m, *args, *((c["ry"], c["held_y"]) if want_y else ()))
            got = _hold_device(h, c, pos, m, Tm, want_y)
            _same(got, want)
            assert set(got) == set(want) and not got["flags"].any() and got["solved"].sum() == m
            if m == 0:                                                       # the case has what H2 is about: both clips and a kept -0.0
                assert (c["held_x"] > c["ub"]).any() and (c["held_x"] < c["lb"]).any() and np.signbit(want["x"][want["x"] == 0]).any()
            held = got["x"][pos < 0]
            assert (held >= c["lb"][pos < 0]).all() and (held <= c["ub"][pos < 0]).all()     # the invariant of a solver output
            # H3: a row that is neither -1 nor a row is held and flagged (device entry: the host entry refuses such a pos)
            bad = pos.copy()
            bad[1], bad[B - 2] = -2, m
            got = _hold_device(h, c, bad, m, Tm, want_y)
            _same(got, spec.hold(bad, m, *args, *((c["ry"], c["held_y"]) if want_y else ())))
            assert got["flags"][1] == got["flags"][B - 2] == spec.HOLD_BAD_ROW and got["flags"].sum() == 2
            # the host entry: the device entry's bits, at any chunking
            for chunk in (None, "2"):
                monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False) if chunk is None else monkeypatch.setenv("ACNQP_POST_CHUNK", chunk)
                host = h.hold_host(pos, m, *args, *((c["ry"], c["held_y"]) if want_y else ()))
                _same(host, want)
            monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False)


def test_select_then_hold_is_the_identity_on_the_device():
    """what the loop does with a step's answers, without a solve in between: x and y come back bit for bit"""
    import torch

    h = _handle("n65_all")
    Tm, K = 12, 1
    dev = torch.device("cuda", 0)
    cur, _, _ = _state(h.site, Tm, K, seed=5)
    rng = np.random.default_rng(6)
    x, y = rng.uniform(cur["lb"], np.maximum(cur["lb"], cur["ub"])), rng.normal(size=(B, h.site.Mg, Tm))
    st = _upload(h, cur, Tm, K, want_y=True)
    idx = [0, 3, 4]
    wx, wy = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    dense = _poisoned(h, Tm, K, want_y=True)
    flags, solved = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    h.select_device(st, dense, torch.tensor(idx, dtype=torch.int32, device=dev), flags, 3, warm_x=wx, warm_y=wy, out_warm_x=dense.x, out_warm_y=dense.y)
    dense.status.fill_(1)
    dense.iters.fill_(9)
    prev = torch.full((B,), 5, dtype=torch.int32, device=dev)
    h.hold_device(st, dense.head(3), torch.from_numpy(spec.inverse(idx, B)).to(dev), 3, wx, prev, solved, flags, held_y=wy)
    torch.cuda.synchronize(dev)
    held = np.setdiff1d(np.arange(B), idx)
    assert np.array_equal(_bits(st.x.cpu().numpy()[idx]), _bits(x[idx])) and np.array_equal(_bits(st.y.cpu().numpy()), _bits(y))
    clipped = np.where(x > cur["ub"], cur["ub"], x)
    clipped = np.where(clipped < cur["lb"], cur["lb"], clipped)
    assert np.array_equal(_bits(st.x.cpu().numpy()[held]), _bits(clipped[held]))
    assert list(st.status.cpu().numpy()) == [1, 5, 5, 1, 1] and list(st.iters.cpu().numpy()) == [9, 0, 0, 9, 9]
    assert list(solved.cpu().numpy()) == [1, 0, 0, 1, 1] and not flags.cpu().numpy().any()


def test_bad_arguments_are_refused_before_any_device_work():
    import torch
    from adacharge_amd import backend

    lib = backend.load_library()
    h = _handle("n3_all")
    site, Tm, K, m = h.site, 12, 2, 3
    N, Mg = site.N, site.Mg
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur, wx, wy = _state(site, Tm, K, seed=3)
    st, dense = _upload(h, cur, Tm, K, want_y=True), _poisoned(h, Tm, K, want_y=True)
    for k in ("x", "status", "iters", "y"):                                  # (the results of the state are outputs of hold)
        getattr(st, k).fill_(POISON.get(k, float("nan")))
    idx, pos = np.array(IDX[m], np.int32), spec.inverse(IDX[m], B)
    t = dict(idx=up(idx), pos=up(pos), wx=up(wx), wy=up(wy), owx=torch.full((B, N, Tm), float("nan"), dtype=torch.float64, device=dev),
             owy=torch.full((B, Mg, Tm), float("nan"), dtype=torch.float64, device=dev), flags=torch.full((B,), -7, dtype=torch.int32, device=dev),
             solved=torch.full((B,), 77, dtype=torch.uint8, device=dev), prev=up(np.ones(B, np.int32)))
    P, NX = tuple(backend._PROBLEM_ARRAYS), backend._NEXT_ARRAYS
    ptr = lambda v: None if v is None else (C.c_void_p(v.data_ptr()) if hasattr(v, "data_ptr") else v.ctypes.data_as(C.c_void_p))

    def select(entry="device", handle=h._h, n_evse=N, n_rows=Mg, m=m, null=(), batch=B, t_max=Tm, k=K, **kw):
        """the C entry itself; ``kw``: cur_<field> / out_<field> / idx / s_eq / flags replaced by a tensor or None"""
        a = {**{"cur_" + f: getattr(st, f) for f in P}, "cur_warm_x": t["wx"], "cur_warm_y": t["wy"], **{"out_" + f: getattr(dense, f) for f in NX},
             "out_warm_x": t["owx"], "out_warm_y": t["owy"], "idx": t["idx"], "s_eq": dense.s_eq, "flags": t["flags"]}
        a.update(kw)
        if entry == "host":
            a["idx"] = a["idx"] if not hasattr(a["idx"], "cpu") else a["idx"].cpu().numpy()
        p = backend._Problems(batch, t_max, k, *[ptr(a["cur_" + f]) for f in P + ("warm_x", "warm_y")])
        nx = backend._Next(*[ptr(a["out_" + f]) for f in NX + ("warm_x", "warm_y")])
        args = [handle, None if "cur" in null else C.byref(p), n_evse, n_rows, m, ptr(a["idx"]), None if "out" in null else C.byref(nx),
                ptr(a["s_eq"]), ptr(a["flags"])]
        return lib.acnqp_select_device(*args, None) if entry == "device" else lib.acnqp_select_host(*args)

    def hold(entry="device", handle=h._h, n_evse=N, n_rows=Mg, m=m, null=(), batch=B, t_max=Tm, k=1, **kw):
        a = dict(lb=st.lb, ub=st.ub, pos=t["pos"], rx=dense.x, rstatus=dense.status, riters=dense.iters, ry=dense.y, held_x=t["wx"], held_y=t["wy"],
                 prev=t["prev"], x=st.x, status=st.status, iters=st.iters, y=st.y, solved=t["solved"], flags=t["flags"])
        a.update(kw)
        if entry == "host":
            a["pos"] = a["pos"] if not hasattr(a["pos"], "cpu") else a["pos"].cpu().numpy()
        p = backend._Problems(batch, t_max, k, lb=ptr(a["lb"]), ub=ptr(a["ub"]))
        r = backend._Results(x=ptr(a["rx"]), status=ptr(a["rstatus"]), iters=ptr(a["riters"]), y=ptr(a["ry"]))
        o = backend._Results(x=ptr(a["x"]), status=ptr(a["status"]), iters=ptr(a["iters"]), y=ptr(a["y"]))
        args = [handle, None if "cur" in null else C.byref(p), n_evse, n_rows, m, ptr(a["pos"]), None if "dense" in null else C.byref(r),
                ptr(a["held_x"]), ptr(a["held_y"]), ptr(a["prev"]), None if "out" in null else C.byref(o), ptr(a["solved"]), ptr(a["flags"])]
        return lib.acnqp_hold_device(*args, None) if entry == "device" else lib.acnqp_hold_host(*args)

    def refused(fn, match, entries=("device", "host"), **kw):
        for entry in entries:
            assert fn(entry, **kw) == -1, (match, entry)                    # ACNQP_ERR_INVALID
            msg = lib.acnqp_last_error().decode()
            assert match in msg and f"acnqp_{fn.__name__}_{entry}" in msg, (match, msg)

    for fn in (select, hold):
        refused(fn, "null handle", handle=None)
        refused(fn, "null argument", null=("cur",))
        refused(fn, "null argument", null=("out",))
        refused(fn, f"the call is for 4 EVSEs and {Mg} site rows, the handle's site has 3 and {Mg}", n_evse=4)
        refused(fn, f"the call is for 3 EVSEs and {Mg + 1} site rows", n_rows=Mg + 1)
        refused(fn, "negative batch", batch=-1)
        refused(fn, "t_max must be in [1, 4096]", t_max=0)
        refused(fn, "t_max must be in [1, 4096]", t_max=4097)
        refused(fn, "k_sessions must be in [1, 4096]", k=0)
        refused(fn, "m is -1, it must be in [0, batch = 5]", m=-1)
        refused(fn, "m is 6, it must be in [0, batch = 5]", m=6)
    refused(hold, "null argument", null=("dense",))
    # select: required arrays, the arrays of the site's rows, the warm pair, overlaps
    for k in ("cur_horizon", "cur_lb", "cur_ub", "cur_q", "cur_pdiag", "cur_s_off", "cur_s_len", "cur_s_cap", "cur_s_eq", "idx"):
        refused(select, "null problem array or idx", **{k: None})
    for k in ("out_horizon", "out_lb", "out_ub", "out_q", "out_pdiag", "out_s_off", "out_s_len", "out_s_cap", "s_eq", "flags"):
        refused(select, "null output array, s_eq or flags", **{k: None})
    for k in ("cur_peak", "out_peak"):
        refused(select, "site has a peak row but peak is null", **{k: None})
    for k in ("cur_lf", "out_lf"):
        refused(select, "site has a flat row but lf is null", **{k: None})
    for k in ("cur_dc", "out_dc", "cur_dfloor", "out_dfloor"):
        refused(select, "site has a max row but dc or dfloor is null", **{k: None})
    refused(select, "warm_x and warm_y go together on a site with rows", out_warm_y=None)
    refused(select, "warm_x and warm_y go together on a site with rows", out_warm_x=None)
    refused(select, "a warm output is wanted but cur's warm_x or warm_y is null", cur_warm_x=None)
    refused(select, "a warm output is wanted but cur's warm_x or warm_y is null", cur_warm_y=None)
    refused(select, "an output aliases an input (lb overlaps cur->lb)", entries=("device",), out_lb=st.lb)
    refused(select, "an output aliases an input (warm_x overlaps cur->warm_x)", entries=("device",), out_warm_x=t["wx"])
    refused(select, "an output aliases an input (flags overlaps idx)", entries=("device",), flags=t["idx"])
    refused(select, "two outputs overlap (lb and ub)", entries=("device",), out_ub=dense.lb)
    refused(select, "two outputs overlap (horizon and flags)", entries=("device",), flags=dense.horizon)
    refused(select, "idx is not strictly increasing (idx[2] = 2 after 2)", entries=("host",), idx=np.array([0, 2, 2], np.int32))
    refused(select, "idx is not strictly increasing (idx[1] = 0 after 4)", entries=("host",), idx=np.array([4, 0, 2], np.int32))
    # hold: required arrays, y, overlaps, pos
    for k in ("lb", "ub", "pos", "held_x", "prev"):
        refused(hold, "null lb, ub, pos, held_x or prev_status", **{k: None})
    for k in ("x", "status", "iters", "solved", "flags"):
        refused(hold, "null output array, solved or flags", **{k: None})
    for k in ("rx", "rstatus", "riters"):
        refused(hold, "null x, status or iters of the dense results", **{k: None})
    for k in ("held_y", "ry"):
        refused(hold, "y is wanted but held_y or the dense results' y is null", **{k: None})
    refused(hold, "an output aliases an input (x overlaps held_x)", entries=("device",), x=t["wx"])
    refused(hold, "an output aliases an input (x overlaps dense->x)", entries=("device",), x=dense.x)
    refused(hold, "an output aliases an input (status overlaps prev_status)", entries=("device",), status=t["prev"])
    refused(hold, "an output aliases an input (x overlaps cur->ub)", entries=("device",), x=st.ub)
    refused(hold, "two outputs overlap (status and iters)", entries=("device",), iters=st.status)
    refused(hold, "two outputs overlap (status and flags)", entries=("device",), flags=st.status)
    refused(hold, "pos is not the inverse of a strictly increasing idx (pos[0] = 1, the next row is 0)", entries=("host",),
            pos=np.array([1, -1, 0, -1, 2], np.int32))
    refused(hold, "pos is not the inverse of a strictly increasing idx (it names 2 of the 3 rows)", entries=("host",),
            pos=np.array([0, -1, 1, -1, -1], np.int32))
    refused(hold, "pos is not the inverse of a strictly increasing idx (pos[4] = 1, the next row is 2)", entries=("host",),
            pos=np.array([0, -1, 1, -1, 1], np.int32))
    with pytest.raises(ValueError, match="m is 6"):                         # and through the binding
        h.select_device(st, backend.DeviceBatch.empty(site, 8, Tm, K, dev), torch.zeros(8, dtype=torch.int32, device=dev),
                        torch.zeros(8, dtype=torch.int32, device=dev), 6)
    # nothing ran: every output still holds its poison
    torch.cuda.synchronize(dev)
    for k in NX:
        assert _untouched(getattr(dense, k), k), k
    for k in ("x", "status", "iters", "y"):
        assert _untouched(getattr(st, k), k) and _untouched(getattr(dense, k), k), k
    assert np.isnan(t["owx"].cpu().numpy()).all() and np.isnan(t["owy"].cpu().numpy()).all()
    assert (t["flags"].cpu().numpy() == -7).all() and (t["solved"].cpu().numpy() == 77).all() and _untouched(dense.s_eq, "s_eq")
    # two valid calls: select with m == 0 launches nothing (with or without arrays); hold with m == 0 holds everyone
    for entry in ("device", "host"):
        assert select(entry, m=0) == 0 and select(entry, m=0, idx=None, out_lb=None, flags=None) == 0
        assert select(entry, batch=0, m=0) == 0 and hold(entry, batch=0, m=0) == 0
    torch.cuda.synchronize(dev)
    assert _untouched(dense.lb, "lb") and (t["flags"].cpu().numpy() == -7).all()
    assert hold("device", m=0, pos=up(np.full(B, -1, np.int32)), rx=None, rstatus=None, riters=None, ry=None) == 0
    torch.cuda.synchronize(dev)
    want = spec.hold(np.full(B, -1, np.int32), 0, None, None, None, wx, np.ones(B, np.int32), cur["lb"], cur["ub"], None, wy)
    got = dict(x=st.x.cpu().numpy(), y=st.y.cpu().numpy(), status=st.status.cpu().numpy(), iters=st.iters.cpu().numpy(),
               solved=t["solved"].cpu().numpy(), flags=t["flags"].cpu().numpy())
    _same(got, want)
    assert not got["solved"].any()
