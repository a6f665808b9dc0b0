"""The prepare kernel (acnqp_prepare_device / acnqp_prepare_host) returns the bits of tests/prepare_spec.py on the random
pools of tests/prepare_cases.py -- every shape at which the kernel takes another path: one wavefront (54 x 12, 5 x 3, the
edge 64 x 2) and four (65 x 2, 128 x 4) -- writes every view element and flag, leaves the other periods of lb and ub alone,
gives a problem the same bits alone and at any position of a batch, and refuses bad arguments with ACNQP_ERR_INVALID and a
message before any device work.  No solve: the states are random."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import prepare_cases as cases, prepare_spec as spec

pytestmark = pytest.mark.gpu
OUT = ("lb", "ub", "v_evse", "v_arrived", "v_cap", "flags")
_HANDLES = {}


def _handle(name):
    if name not in _HANDLES:
        _HANDLES[name] = cases.handle_of(cases.site_of(name))
    return _HANDLES[name]


@functools.lru_cache(maxsize=None)
def _case(name, Tm):
    """the pool of a shape and the specification's answers (with minimum rates, and the view alone), computed once"""
    pool = cases.random_pool(name, Tm)
    s = pool["site"]
    return pool, spec.prepare(pool["cur"], pool["key"], **s), spec.prepare(pool["cur"], pool["key"], s["cre"], s["cim"], s["limits"], None)


def _device(h, pool, want_view=True, min_rates=True):
    """acnqp_prepare_device on poisoned outputs: dict of numpy arrays"""
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = torch.device("cuda", 0)
    c = pool["cur"]
    B, N, Tm = c["lb"].shape
    cur = DeviceBatch.empty(h.site, B, Tm, 1, dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for k in ("lb", "ub", "s_off", "s_len", "s_cap"):
        getattr(cur, k).copy_(up(c[k]))
    ve = torch.full((B, N), -7, dtype=torch.int32, device=dev) if want_view else None
    va = torch.full((B, N), 249, dtype=torch.uint8, device=dev) if want_view else None
    vc = torch.full((B, N), float("nan"), dtype=torch.float64, device=dev) if want_view else None
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    h.prepare_device(cur, cases.plan_of(pool).to_device(dev), flags, ve, va, vc, min_rates=min_rates)
    torch.cuda.synchronize(dev)
    for k in ("s_off", "s_len", "s_cap"):
        assert np.array_equal(getattr(cur, k).cpu().numpy(), c[k])      # the slot state is read only
    out = dict(lb=cur.lb.cpu().numpy(), ub=cur.ub.cpu().numpy(), flags=flags.cpu().numpy())
    if want_view:
        out.update(v_evse=ve.cpu().numpy(), v_arrived=va.cpu().numpy(), v_cap=vc.cpu().numpy())
    return out


def _same(got, want, keys=OUT):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name,Tm", cases.SHAPES)
def test_device_and_host_equal_spec_bit_for_bit(name, Tm):
    pool, want, want_view = _case(name, Tm)
    h = _handle(name)
    c = pool["cur"]
    assert c["lb"].shape[0] == 7
    acc = want["accepted"]
    assert (acc == 1).any() and (acc == 0).any() and (acc == -1).any() and want["flags"].tolist() == [0, 0, 0, 0, 0, 1, 0]
    assert (want["lb"][:, :, 0] != c["lb"][:, :, 0]).any() and (want["ub"][:, :, 0] != c["ub"][:, :, 0]).any()
    assert np.array_equal(want["lb"][:, :, 1:], c["lb"][:, :, 1:]) and np.array_equal(want["ub"][:, :, 1:], c["ub"][:, :, 1:])
    _same(_device(h, pool), want)                                       # (array_equal on the whole of lb and ub: the untouched periods too)
    _same(h.prepare_host(c, cases.plan_of(pool)), want)
    # no minimum rates: the bounds stay, the view reads them as they are
    assert np.array_equal(want_view["lb"], c["lb"]) and np.array_equal(want_view["ub"], c["ub"])
    _same(_device(h, pool, min_rates=False), want_view)
    _same(h.prepare_host(c, cases.plan_of(pool), min_rates=False), want_view)
    # no view: the same bounds and flags
    _same(_device(h, pool, want_view=False), want, ("lb", "ub", "flags"))
    _same(h.prepare_host(c, cases.plan_of(pool), want_view=False), want, ("lb", "ub", "flags"))


@pytest.mark.parametrize("name,Tm", cases.SHAPES)
def test_same_bits_alone_and_at_any_position(name, Tm):
    pool, want, _ = _case(name, Tm)
    h = _handle(name)
    alone = _device(h, cases.subset(pool, 2))
    for k in OUT:
        assert np.array_equal(alone[k][0], want[k][2]), k
    moved = dict(pool, cur={k: v.copy() for k, v in pool["cur"].items()}, key=pool["key"].copy())
    for pos in (0, 3, 6):
        for k in moved["cur"]:
            moved["cur"][k][pos] = pool["cur"][k][2]
        moved["key"][pos] = pool["key"][2]
    got = _device(h, moved)
    for pos in (0, 3, 6):
        for k in OUT:
            assert np.array_equal(got[k][pos], alone[k][0]), (pos, k)
    for k in OUT:                                                        # and the problems in between are their own
        assert np.array_equal(got[k][1], want[k][1]) and np.array_equal(got[k][5], want[k][5]), k


def test_host_entry_in_chunks_of_3_3_1_in_a_child_process(tmp_path):
    name, Tm = cases.SHAPES[0]
    pool, want, _ = _case(name, Tm)
    one = _handle(name).prepare_host(pool["cur"], cases.plan_of(pool))
    out = str(tmp_path / "chunked.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-m", "tests.prepare_cases", name, str(Tm), out], cwd=root, check=True, timeout=120,
                   env=dict(os.environ, ACNQP_POST_CHUNK="3"))
    got = dict(np.load(out))
    _same(got, one)
    _same(got, want)


def test_bad_arguments_are_refused_before_any_device_work():
    import torch
    from adacharge_amd import backend
    from adacharge_amd.backend import DeviceBatch

    lib = backend.load_library()
    name, Tm = cases.SHAPES[0]
    pool, _, _ = _case(name, Tm)
    h = _handle(name)
    dev = torch.device("cuda", 0)
    c = pool["cur"]
    B, N, _ = c["lb"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def state(K=1):
        cur = DeviceBatch.empty(h.site, B, Tm, K, dev)
        for k in ("lb", "ub"):
            getattr(cur, k).copy_(up(c[k]))
        if K == 1:
            for k in ("s_off", "s_len", "s_cap"):
                getattr(cur, k).copy_(up(c[k]))
        return cur

    cur = state()
    plan = cases.plan_of(pool).to_device(dev)
    ve = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    va = torch.full((B, N), 249, dtype=torch.uint8, device=dev)
    vc = torch.full((B, N), float("nan"), dtype=torch.float64, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)

    def refused(match, **kw):
        args = dict(cur=cur, plan=plan, flags=flags, v_evse=ve, v_arrived=va, v_cap=vc)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            h.prepare_device(**args)
        assert lib.acnqp_last_error() != b""

    refused("k_sessions must be 1", cur=state(K=2))
    refused("a view needs", v_cap=None)
    refused("a view needs", v_evse=None)
    other = backend.PreparePlan(key=plan.key, cre=plan.cre[:5].contiguous(), cim=plan.cim[:5].contiguous(), limits=plan.limits[:5].contiguous(),
                                min_pilot=plan.min_pilot)
    refused("the handle's site has 54 and 8", plan=other)                                   # n_infra other than the handle's
    with pytest.raises(ValueError, match="the handle's site has 5 and 7"):                  # n_evse other than the handle's
        _handle("five").prepare_device(cur, plan, flags, ve, va, vc)
    half = state()
    half.ub = half.lb                                                                     # two outputs in one buffer
    refused("two outputs overlap", cur=half)
    alias = backend.PreparePlan(key=ve, cre=plan.cre, cim=plan.cim, limits=plan.limits, min_pilot=plan.min_pilot)
    refused("v_evse overlaps key", plan=alias)                                              # an output over an input
    alias = backend.PreparePlan(key=plan.key, cre=plan.cre, cim=plan.cim, limits=plan.limits, min_pilot=vc[0].contiguous())
    refused("v_cap overlaps min_pilot", plan=alias)
    refused("flags overlaps s_len", flags=cur.s_len.view(-1)[:B])
    p = backend._Problems(B, Tm, 1, *[None] * 15)
    pl = plan._struct(N)
    view = backend._PrepareView()
    assert lib.acnqp_prepare_device(None, C.byref(p), C.byref(pl), None, None, C.byref(view), None, None) == -1
    assert b"null handle" in lib.acnqp_last_error()
    assert lib.acnqp_prepare_host(None, C.byref(p), C.byref(pl), None, None, C.byref(view), None) == -1
    assert b"null handle" in lib.acnqp_last_error()
    assert lib.acnqp_prepare_device(h._h, C.byref(p), C.byref(pl), None, None, C.byref(view), None, None) == -1
    assert b"null slot array" in lib.acnqp_last_error()
    torch.cuda.synchronize(dev)
    assert (flags.cpu().numpy() == -7).all() and (ve.cpu().numpy() == -7).all() and (va.cpu().numpy() == 249).all()   # nothing ran
    assert np.isnan(vc.cpu().numpy()).all()
    assert np.array_equal(cur.lb.cpu().numpy(), c["lb"]) and np.array_equal(cur.ub.cpu().numpy(), c["ub"])
