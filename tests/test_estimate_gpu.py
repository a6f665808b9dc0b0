"""The estimator kernel (acnqp_estimate_device / acnqp_estimate_host) returns the bits of tests/estimate_spec.py on the calls
of tests/estimate_cases.py -- N in {1, 54, 64, 65, 130}: one wavefront, its edge, four, and the loop beyond 64 lanes of one;
B in {1, 3, 257}; Tm in {1, 5, 12} -- with every branch of the rules in every shape (asserted on the CPU,
tests/test_estimate_spec.py), with and without ``status`` and ``actual``, writes every output whatever the input, leaves its
inputs alone, gives a problem the same bits alone and at three positions of a batch of 257, gives the host entry's bits at
any chunking, and refuses bad arguments with ACNQP_ERR_INVALID and a message before any device work.  No solve: the states
are synthetic."""
import ctypes as C

import numpy as np
import pytest

from tests import estimate_cases as cases

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_library")]
OUT = ("est", "ub", "flags")
PARAMS = dict(up_threshold=cases.UP, down_threshold=cases.DOWN, up_increment=cases.INC)
_HANDLES = {}


def _handle(N):
    if N not in _HANDLES:
        _HANDLES[N] = cases.handle_of(N)
    return _HANDLES[N]


def _device(h, call):
    """acnqp_estimate_device on poisoned outputs: dict of numpy arrays"""
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = torch.device("cuda", 0)
    B, N, Tm = call["cur"]["ub"].shape
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur = DeviceBatch.empty(h.site, B, Tm, 1, dev)
    for k, v in call["cur"].items():
        getattr(cur, k).copy_(up(v))
    fresh, pilots, actual, status, est = (up(call[k]) for k in ("fresh", "pilots", "actual", "status", "est"))
    ub_out = torch.full((B, N, Tm), float("nan"), dtype=torch.float64, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    h.estimate_device(cur, fresh, est, ub_out, flags, pilots=pilots, actual=actual, status=status, **PARAMS)
    torch.cuda.synchronize(dev)
    for got, want in tuple((getattr(cur, k), v) for k, v in call["cur"].items()) + ((fresh, call["fresh"]), (pilots, call["pilots"]),
                                                                                 (actual, call["actual"]), (status, call["status"])):
        assert got is None or np.array_equal(got.cpu().numpy(), want)           # the inputs are read only
    return dict(est=est.cpu().numpy(), ub=ub_out.cpu().numpy(), flags=flags.cpu().numpy())


def _same(got, want):
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


def _full(calls):
    """the first call with the whole history"""
    return next(c for c in calls if c["pilots"] is not None and c["actual"] is not None)


@pytest.mark.parametrize("Tm", cases.TMS)
@pytest.mark.parametrize("B", cases.BS)
@pytest.mark.parametrize("N", cases.NS)
def test_device_equals_spec_bit_for_bit(N, B, Tm):
    h = _handle(N)
    calls, want = cases.calls(N, B, Tm), cases.answers(N, B, Tm)
    assert len(calls) == cases.n_calls(N, B)
    for c, w in zip(calls, want):
        _same(_device(h, c), w)
    # the same state with less history: no status (every problem is served), no actual (what is offered is drawn), neither
    c = _full(calls)
    for less in (dict(status=None), dict(actual=None), dict(status=None, actual=None)):
        _same(_device(h, dict(c, **less)), cases.run_spec(c, **less))


@pytest.mark.parametrize("N", cases.NS)
def test_same_bits_alone_and_at_three_positions_of_257(N):
    Tm = 12
    h = _handle(N)
    small, big = _full(cases.calls(N, 3, Tm)), _full(cases.calls(N, 257, Tm))
    flat = ("fresh", "est", "pilots", "actual", "status")
    pick = lambda c, b: dict(cur={k: np.ascontiguousarray(v[b:b + 1]) for k, v in c["cur"].items()},
                             **{k: np.ascontiguousarray(c[k][b:b + 1]) for k in flat})
    alone = _device(h, pick(small, 2))
    want_small = cases.run_spec(small)
    for k in OUT:
        assert np.array_equal(alone[k][0], want_small[k][2]), k
    moved = dict(cur={k: v.copy() for k, v in big["cur"].items()}, **{k: big[k].copy() for k in flat})
    spots = (0, 100, 256)
    for pos in spots:
        for k in moved["cur"]:
            moved["cur"][k][pos] = small["cur"][k][2]
        for k in flat:
            moved[k][pos] = small[k][2]
    got = _device(h, moved)
    want = cases.run_spec(big)
    rest = np.setdiff1d(np.arange(257), spots)
    for k in OUT:
        for pos in spots:
            assert np.array_equal(got[k][pos], alone[k][0]), (pos, k)
        assert np.array_equal(got[k][rest], want[k][rest]), k              # and the problems in between are their own


@pytest.mark.parametrize("N,B,Tm", [(N, 3, 5) for N in cases.NS] + [(54, 257, 12), (130, 257, 1)])
def test_host_entry_equals_device_entry_at_any_chunking(N, B, Tm, monkeypatch):
    h = _handle(N)
    c = _full(cases.calls(N, B, Tm))
    est_before = c["est"].copy()
    one = _device(h, c)
    _same(one, cases.run_spec(c))
    host = lambda c: h.estimate_host(c["cur"], c["fresh"], c["est"], pilots=c["pilots"], actual=c["actual"], status=c["status"], **PARAMS)
    for chunk in (None, "1", "2"):
        if chunk is None:
            monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False)
        else:
            monkeypatch.setenv("ACNQP_POST_CHUNK", chunk)
        _same(host(c), one)
    monkeypatch.setenv("ACNQP_POST_CHUNK", "2")
    for less in (dict(status=None, actual=None), dict(status=None, actual=None, pilots=None)):
        _same(host(dict(c, **less)), cases.run_spec(c, **less))
    assert np.array_equal(c["est"], est_before)                              # the host entry works on a copy of est


def test_a_fresh_block_per_step_is_picked_by_fresh_row():
    import torch

    N, B, Tm = 54, 3, 5
    h = _handle(N)
    c = _full(cases.calls(N, B, Tm))
    rows = np.stack([np.zeros_like(c["fresh"]), c["fresh"], 1 - c["fresh"]])
    want = cases.run_spec(c)
    _same(h.estimate_host(c["cur"], rows, c["est"], pilots=c["pilots"], actual=c["actual"], status=c["status"], fresh_row=1, **PARAMS), want)
    _same(_device(h, dict(c, fresh=rows[2])), cases.run_spec(c, fresh=rows[2]))
    from adacharge_amd.backend import DeviceBatch

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur = DeviceBatch.empty(h.site, B, Tm, 1, dev)
    for k, v in c["cur"].items():
        getattr(cur, k).copy_(up(v))
    est, ub_out, flags = up(c["est"]), torch.zeros((B, N, Tm), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    h.estimate_device(cur, up(rows), est, ub_out, flags, pilots=up(c["pilots"]), actual=up(c["actual"]), status=up(c["status"]), fresh_row=1,
                      **PARAMS)
    torch.cuda.synchronize(dev)
    _same(dict(est=est.cpu().numpy(), ub=ub_out.cpu().numpy(), flags=flags.cpu().numpy()), want)
    with pytest.raises(ValueError, match="fresh_row is outside fresh"):
        h.estimate_device(cur, up(rows), est, ub_out, flags, fresh_row=3, **PARAMS)


def test_bad_arguments_are_refused_before_any_device_work():
    import torch
    from adacharge_amd import backend
    from adacharge_amd.backend import DeviceBatch

    lib = backend.load_library()
    N, B, Tm = 54, 3, 5
    h = _handle(N)
    c = _full(cases.calls(N, B, Tm))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur = DeviceBatch.empty(h.site, B, Tm, 1, dev)
    for k, v in c["cur"].items():
        getattr(cur, k).copy_(up(v))
    t = dict(fresh=up(c["fresh"]), pilots=up(c["pilots"]), actual=up(c["actual"]), status=up(c["status"]), est=up(c["est"]),
             ub_out=torch.full((B, N, Tm), float("nan"), dtype=torch.float64, device=dev), flags=torch.full((B,), -7, dtype=torch.int32, device=dev),
             s_off=cur.s_off, s_len=cur.s_len, lb=cur.lb, ub=cur.ub)

    def raw(entry="device", handle=h._h, batch=B, K=1, t_max=Tm, null_cur=False, **kw):
        """the C entry itself: a name in ``kw`` replaces that argument (a tensor, or None for NULL)"""
        a = dict(t)
        a.update(kw)
        p = backend._Problems(batch, t_max, K, **{k: backend._dptr(a[k]) for k in ("s_off", "s_len", "lb", "ub")})
        args = ([handle, None if null_cur else C.byref(p)] + [backend._dptr(a[k]) for k in ("fresh", "pilots", "actual", "status")]
                + [C.c_double(v) for v in (cases.UP, cases.DOWN, cases.INC)] + [backend._dptr(a[k]) for k in ("est", "ub_out", "flags")])
        fn = lib.acnqp_estimate_device if entry == "device" else lib.acnqp_estimate_host
        return fn(*args, *((None,) if entry == "device" else ()))

    def refused(match, **kw):
        for entry in ("device", "host"):
            assert raw(entry, **kw) == -1, (match, entry)                 # ACNQP_ERR_INVALID
            msg = lib.acnqp_last_error().decode()
            assert match in msg and f"acnqp_estimate_{entry}" in msg, (match, msg)

    refused("null handle", handle=None)
    refused("null argument", null_cur=True)
    for k in ("s_off", "s_len", "lb", "ub", "fresh", "est", "ub_out", "flags"):
        refused("null slot array, lb, ub, fresh, est, ub_out or flags", **{k: None})
    refused("k_sessions must be 1", K=2)
    refused("negative batch", batch=-1)
    refused("t_max must be in [1, 4096]", t_max=0)
    refused("actual is given without pilots", pilots=None)
    refused("an output aliases an input (ub_out overlaps ub)", ub_out=t["ub"])
    refused("ub_out overlaps lb", ub_out=t["lb"])
    refused("est overlaps pilots", est=t["pilots"])
    refused("est overlaps actual", est=t["actual"])
    refused("flags overlaps status", flags=t["status"])
    refused("flags overlaps fresh", flags=t["fresh"].view(-1)[7:])
    refused("flags overlaps s_len", flags=t["s_len"].view(-1)[2:])
    refused("two outputs overlap (est and ub_out)", est=t["ub_out"].view(-1)[B * N * (Tm - 1):])
    refused("two outputs overlap (est and flags)", flags=t["est"].view(torch.int32).view(-1)[4:])
    with pytest.raises(ValueError, match="k_sessions must be 1"):         # and through the binding
        h.estimate_device(DeviceBatch.empty(h.site, B, Tm, 2, dev), t["fresh"], t["est"], t["ub_out"], t["flags"])
    with pytest.raises(ValueError, match="ub_out overlaps ub"):
        h.estimate_device(cur, t["fresh"], t["est"], cur.ub, t["flags"])
    with pytest.raises(ValueError, match="actual is given without pilots"):
        h.estimate_device(cur, t["fresh"], t["est"], t["ub_out"], t["flags"], actual=t["actual"])
    # an empty batch is no error, with or without arrays
    for entry in ("device", "host"):
        assert raw(entry, batch=0) == 0
        assert raw(entry, batch=0, fresh=None, est=None, ub_out=None) == 0
    torch.cuda.synchronize(dev)
    assert np.isnan(t["ub_out"].cpu().numpy()).all() and (t["flags"].cpu().numpy() == -7).all()   # nothing ran
    assert np.array_equal(t["est"].cpu().numpy(), c["est"]) and np.array_equal(cur.ub.cpu().numpy(), c["cur"]["ub"])
