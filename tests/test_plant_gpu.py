"""The plant kernel (acnqp_plant_device / acnqp_plant_host) returns the bits of tests/plant_spec.py on the calls of
tests/plant_cases.py -- N in {1, 54, 64, 65, 130}: one wavefront, its edge, four, and the loop beyond 64 lanes of one;
B in {1, 3, 257} -- with every branch of the rules in every shape (asserted on the CPU, tests/test_plant_spec.py), writes
every output whatever the input, leaves its inputs alone, gives a problem the same bits alone and at three positions of a
batch of 257, gives the host entry's bits at any chunking, and refuses bad arguments with ACNQP_ERR_INVALID and a message
before any device work.  No solve: the states are synthetic."""
import ctypes as C

import numpy as np
import pytest

from tests import plant_cases as cases, plant_spec as spec

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("hip_library")]
OUT = ("bat", "room", "actual", "flags")
_HANDLES = {}


def _handle(N):
    if N not in _HANDLES:
        _HANDLES[N] = cases.handle_of(N)
    return _HANDLES[N]


def _device(h, call, use_status=True):
    """acnqp_plant_device on poisoned outputs: dict of numpy arrays"""
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = torch.device("cuda", 0)
    B, N = call["pilots"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur = DeviceBatch.empty(h.site, B, 1, 1, dev)
    cur.s_off.copy_(up(call["cur"]["s_off"]))
    cur.s_len.copy_(up(call["cur"]["s_len"]))
    plan = cases.plan_of(call).to_device(dev)
    pilots, status, bat, room = up(call["pilots"]), up(call["status"]), up(call["bat"]), up(call["room"])
    actual = torch.full((B, N), float("nan"), dtype=torch.float64, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    h.plant_device(cur, plan, pilots, bat, room, actual, flags, status=status if use_status else None)
    torch.cuda.synchronize(dev)
    for got, want in ((cur.s_off, call["cur"]["s_off"]), (cur.s_len, call["cur"]["s_len"]), (pilots, call["pilots"]), (status, call["status"]),
                      (plan.plug, call["plug"])) + tuple((getattr(plan, k), v) for k, v in cases.table().items()):
        assert np.array_equal(got.cpu().numpy(), want)                   # the inputs are read only
    return dict(bat=bat.cpu().numpy(), room=room.cpu().numpy(), actual=actual.cpu().numpy(), flags=flags.cpu().numpy())


def _same(got, want):
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("B", cases.BS)
@pytest.mark.parametrize("N", cases.NS)
def test_device_equals_spec_bit_for_bit(N, B):
    h = _handle(N)
    calls, want = cases.calls(N, B), cases.answers(N, B)
    assert len(calls) == cases.n_calls(N, B)
    for c, w in zip(calls, want):
        _same(_device(h, c), w)
    # no status: every problem is served
    c = calls[-1]
    _same(_device(h, c, use_status=False), spec.plant(c["cur"], c["pilots"], None, cases.table(), c["plug"], c["bat"], c["room"]))


@pytest.mark.parametrize("N", cases.NS)
def test_same_bits_alone_and_at_three_positions_of_257(N):
    h = _handle(N)
    small, big = cases.calls(N, 3)[0], cases.calls(N, 257)[0]
    pick = lambda c, b: dict(cur={k: np.ascontiguousarray(v[b:b + 1]) for k, v in c["cur"].items()},
                             **{k: np.ascontiguousarray(c[k][b:b + 1]) for k in ("pilots", "status", "plug", "bat", "room")})
    alone = _device(h, pick(small, 2))
    for k in OUT:
        assert np.array_equal(alone[k][0], cases.answers(N, 3)[0][k][2]), k
    moved = dict(cur={k: v.copy() for k, v in big["cur"].items()}, **{k: big[k].copy() for k in ("pilots", "status", "plug", "bat", "room")})
    spots = (0, 100, 256)
    for pos in spots:
        for k in moved["cur"]:
            moved["cur"][k][pos] = small["cur"][k][2]
        for k in ("pilots", "status", "plug", "bat", "room"):
            moved[k][pos] = small[k][2]
    got = _device(h, moved)
    want = cases.answers(N, 257)[0]
    rest = np.setdiff1d(np.arange(257), spots)
    for k in OUT:
        for pos in spots:
            assert np.array_equal(got[k][pos], alone[k][0]), (pos, k)
        assert np.array_equal(got[k][rest], want[k][rest]), k              # and the problems in between are their own


@pytest.mark.parametrize("N,B", [(N, 3) for N in cases.NS] + [(54, 257), (130, 257)])
def test_host_entry_equals_device_entry_at_any_chunking(N, B, monkeypatch):
    h = _handle(N)
    c = cases.calls(N, B)[0]
    one = _device(h, c)
    _same(one, cases.answers(N, B)[0])
    for chunk in (None, "1", "2"):
        if chunk is None:
            monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False)
        else:
            monkeypatch.setenv("ACNQP_POST_CHUNK", chunk)
        _same(h.plant_host(c["cur"], cases.plan_of(c), c["pilots"], c["bat"], c["room"], status=c["status"]), one)
    monkeypatch.delenv("ACNQP_POST_CHUNK", raising=False)
    none = h.plant_host(c["cur"], cases.plan_of(c), c["pilots"], c["bat"], c["room"])
    _same(none, spec.plant(c["cur"], c["pilots"], None, cases.table(), c["plug"], c["bat"], c["room"]))


def test_bad_arguments_are_refused_before_any_device_work():
    import torch
    from adacharge_amd import backend
    from adacharge_amd.backend import DeviceBatch

    lib = backend.load_library()
    N, B = 54, 3
    h = _handle(N)
    c = cases.calls(N, B)[0]
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cur = DeviceBatch.empty(h.site, B, 1, 1, dev)
    cur.s_off.copy_(up(c["cur"]["s_off"]))
    cur.s_len.copy_(up(c["cur"]["s_len"]))
    plan = cases.plan_of(c).to_device(dev)
    t = dict(pilots=up(c["pilots"]), status=up(c["status"]), bat=up(c["bat"]), room=up(c["room"]),
             actual=torch.full((B, N), float("nan"), dtype=torch.float64, device=dev), flags=torch.full((B,), -7, dtype=torch.int32, device=dev),
             t_room=plan.t_room, t_amps=plan.t_amps, t_knee=plan.t_knee, t_slope=plan.t_slope, plug=plan.plug, s_off=cur.s_off, s_len=cur.s_len)
    ORDER = ("pilots", "status", "R", "t_room", "t_amps", "t_knee", "t_slope", "plug", "bat", "room", "actual", "flags")

    def raw(entry="device", handle=h._h, batch=B, K=1, null_cur=False, **kw):
        """the C entry itself: a name in ``kw`` replaces that argument (a tensor, None for NULL, or for R a number)"""
        a = dict(t, R=cases.R)
        a.update(kw)
        p = backend._Problems(batch, 1, K, s_off=backend._dptr(a["s_off"]), s_len=backend._dptr(a["s_len"]))
        args = [handle, None if null_cur else C.byref(p)] + [C.c_int32(a[k]) if k == "R" else backend._dptr(a[k]) for k in ORDER]
        fn = lib.acnqp_plant_device if entry == "device" else lib.acnqp_plant_host
        return fn(*args, *((None,) if entry == "device" else ()))

    def refused(match, **kw):
        for entry in ("device", "host"):
            assert raw(entry, **kw) == -1, (match, entry)                 # ACNQP_ERR_INVALID
            msg = lib.acnqp_last_error().decode()
            assert match in msg and f"acnqp_plant_{entry}" in msg, (match, msg)

    refused("null handle", handle=None)
    refused("null argument", null_cur=True)
    for k in ("pilots", "plug", "bat", "room", "actual", "flags", "s_off", "s_len"):
        refused("null slot array, pilots, plug, bat, room, actual or flags", **{k: None})
    refused("k_sessions must be 1", K=2)
    refused("negative batch", batch=-1)
    refused("negative n_batteries", R=-1)
    for k in ("t_room", "t_amps", "t_knee", "t_slope"):
        refused("n_batteries is 7 but t_room, t_amps, t_knee or t_slope is null", **{k: None})
    refused("actual overlaps pilots", actual=t["pilots"])
    refused("room overlaps pilots", room=t["pilots"])
    refused("flags overlaps status", flags=t["status"])
    refused("bat overlaps plug", bat=t["plug"])
    refused("bat overlaps s_len", bat=t["s_len"])
    refused("an output aliases an input (actual overlaps ", actual=t["t_amps"])   # (3 x 54 doubles from there: t_amps, or a neighbour first)
    refused("flags overlaps t_slope", flags=t["t_slope"][3:])
    refused("two outputs overlap (room and actual)", actual=t["room"])
    refused("two outputs overlap (bat and flags)", flags=t["bat"].view(-1)[5:])
    with pytest.raises(ValueError, match="k_sessions must be 1"):         # and through the binding
        h.plant_device(DeviceBatch.empty(h.site, B, 1, 2, dev), plan, t["pilots"], t["bat"], t["room"], t["actual"], t["flags"])
    with pytest.raises(ValueError, match="actual overlaps pilots"):
        h.plant_device(cur, plan, t["pilots"], t["bat"], t["room"], t["pilots"], t["flags"])
    # an empty batch is no error, with or without arrays; no table at all is none either (every plug is then beyond it)
    for entry in ("device", "host"):
        assert raw(entry, batch=0) == 0
        assert raw(entry, batch=0, pilots=None, bat=None, actual=None) == 0
    torch.cuda.synchronize(dev)
    assert np.isnan(t["actual"].cpu().numpy()).all() and (t["flags"].cpu().numpy() == -7).all()   # nothing ran
    assert np.array_equal(t["bat"].cpu().numpy(), c["bat"]) and np.array_equal(t["room"].cpu().numpy(), c["room"])
    assert np.array_equal(t["pilots"].cpu().numpy(), c["pilots"])
    # n_batteries == 0 with null tables: served; every plug >= 0 and every bat >= 0 is beyond the table
    assert raw("device", R=0, t_room=None, t_amps=None, t_knee=None, t_slope=None) == 0
    torch.cuda.synchronize(dev)
    empty = {k: np.zeros(0) for k in cases.table()}
    want = spec.plant(c["cur"], c["pilots"], c["status"], empty, c["plug"], c["bat"], c["room"])
    _same({k: t[k].cpu().numpy() for k in OUT}, want)
    assert (want["flags"] == 3).any()
