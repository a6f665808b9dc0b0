"""Gradients through the closed loop on the GPU:
  1  acnqp_advance_vjp_device / _host against tests/advance_vjp_spec.py, bit for bit: both block sizes (the launcher takes the
     64-thread kernel up to N = 64 and the 256-thread one beyond: N = 8 and 54 run the first, N = 70 the second), K = 1 and 2,
     with and without the clock cost, step -1, a middle step and a last step without next adjoints, random states and the
     hand cases, host entry = device entry, and 2 CUs + 3 copies of one problem give every copy the same bits
  2  refusals leave poisoned outputs untouched
  3  keep_tape=False and keep_tape=True return the same bits
  4  rollout_gradients against the specification's sweep on the downloaded tape (the device's own answers at every step)
  5  simulate_prices(...).mul(w).sum().backward() gives rollout_gradients(...).prices, bit for bit
  6  a horizon-48 rollout with vjp_long
Measured on an MI355X, (4): worst |kernel - spec|_inf / max(1, |spec|_inf) 3.83e-16 over prices, garr and limits."""
import functools

import numpy as np
import pytest

from adacharge_amd import AdaptiveSchedulingAlgorithm, sites
from adacharge_amd import backend
from adacharge_amd.builder import make_site
from adacharge_amd.rollout import FleetTable, rollout_gradients
from tests import advance_vjp_cases as cases
from tests import rollout_vjp_spec as RS
from tests import test_rollout_vjp_spec as T

pytestmark = pytest.mark.gpu
TIGHT = dict(eps_abs=1e-9, eps_rel=1e-9)
# (4): ten times the worst figure measured on an MI355X, 3.83e-16 (prices 1.7e-16, garr 2.8e-16, limits 3.8e-16: rounding
# level, as the single solve's 5e-15 of DESIGN.md section 3.6i); the figures are printed before they are asserted
E2E_TOL = 3.83e-15


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@functools.lru_cache(maxsize=None)
def handle_for(n):
    infra = sites.caltech54() if n == 54 else sites.balanced_three_phase(n, pods=1, load_fraction=0.35)
    return backend.SiteHandle(make_site(infra, "SOC"), 0)


def plan_of(case, B, N, Tm):
    p, c = case["plan"], case["cost"]
    return backend.AdvancePlan(q_table=np.zeros((1, N, Tm)), h_scal=np.zeros((1, 3)), h_row=np.zeros(Tm + 1, np.int32), done_tol=p["done_tol"],
                               kw_per_amp=0.208, a_seg=p["a_seg"], a_evse=p["a_evse"], a_slot=p["a_slot"], a_len=p["a_len"], a_cap=p["a_cap"],
                               a_rate_seg=p["a_rate_seg"], a_min=p["a_min"], a_max=p["a_max"], c_coef=None if c is None else c["coef"],
                               c_weight=None if c is None else c["weight"], c_series=None if c is None else np.zeros((B, c["series_len"])))


def run_host(handle, case):
    B, K, N = case["cur"]["s_off"].shape
    Tm = case["plan"]["t_max"]
    nxt = case["nxt"] or {}
    return handle.advance_vjp(case["cur"], plan_of(case, B, N, Tm), case["plan"]["step"], applied=case["applied"], status=case["status"],
                              x=case["x"], max_pilot=case["max_pilot"], gdir=case["gdir"], gq_next=nxt.get("gq"),
                              gcap_vjp_next=nxt.get("gcap_vjp"), gcap_carry_next=nxt.get("gcap_carry"), horizon_next=nxt.get("horizon"),
                              flags_next=nxt.get("flags"), garr=case["garr"].copy(), gprice=None if case["gprice"] is None else case["gprice"].copy())


def device_args(handle, case):
    """(cur, plan, keyword tensors) of a case on the device; the outputs start from the case's garr / gprice, gx and
    gcap_carry from a poison value"""
    import torch

    dev = torch.device("cuda", 0)
    B, K, N = case["cur"]["s_off"].shape
    Tm = case["plan"]["t_max"]
    to = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    cur = backend.DeviceBatch.empty(handle.site, B, Tm, K, dev)
    cur.s_off, cur.s_len, cur.s_cap = to(case["cur"]["s_off"], np.int32), to(case["cur"]["s_len"], np.int32), to(case["cur"]["s_cap"])
    if case["x"] is not None:
        cur.x, cur.status = to(case["x"]), to(case["status"], np.int32)
    nxt = case["nxt"] or {}
    at = case["plan"]["step"] >= 0
    kw = dict(applied=to(case["applied"]), max_pilot=to(case["max_pilot"]), gdir=to(case["gdir"]),
              gx=torch.full((B, N, Tm), 7.5, dtype=torch.float64, device=dev) if at else None, gq_next=to(nxt.get("gq")),
              gcap_vjp_next=to(nxt.get("gcap_vjp")), gcap_carry_next=to(nxt.get("gcap_carry")), horizon_next=to(nxt.get("horizon"), np.int32),
              flags_next=to(nxt.get("flags"), np.int32), garr=to(case["garr"]), gprice=to(case["gprice"]))
    carry = torch.full((B, K, N), 7.5, dtype=torch.float64, device=dev)
    return cur, plan_of(case, B, N, Tm).to_device(dev), carry, kw


def run_device(handle, case):
    import torch

    cur, plan, carry, kw = device_args(handle, case)
    handle.advance_vjp_device(cur, plan, case["plan"]["step"], carry, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    out = dict(gcap_carry=carry.cpu().numpy(), garr=kw["garr"].cpu().numpy())
    if kw["gx"] is not None:
        out["gx"] = kw["gx"].cpu().numpy()
    if kw["gprice"] is not None:
        out["gprice"] = kw["gprice"].cpu().numpy()
    return out


def check(case, want, got, what):
    for k in ("gx", "gcap_carry", "garr", "gprice"):
        if want.get(k) is None:   # step -1 writes no gx; without a clock cost there is no gprice
            assert k not in got, (what, k)
            continue
        assert same_bits(want[k], got[k]), (what, k, float(np.abs(want[k] - got[k]).max()))


def test_launcher_switch_is_the_forward_kernels():
    """the forward kernel runs one wavefront up to N = 64 and four beyond (advance_threads, acn_qp_advance.hpp): the adjoint
    is instantiated the same way, so N = 8 and N = 54 run the 64-thread kernel and N = 70 the 256-thread one"""
    import os

    src = open(os.path.join(os.path.dirname(backend.__file__), "csrc", "acn_qp_advance.hpp")).read()
    assert "inline int advance_threads(int N) { return N <= 64 ? 64 : 256; }" in src
    src = open(os.path.join(os.path.dirname(backend.__file__), "csrc", "acn_qp_advance_vjp.hip")).read()
    assert "advance_threads(a.N) == 64" in src


@pytest.mark.parametrize("clock", (True, False))
@pytest.mark.parametrize("K", (1, 2))
@pytest.mark.parametrize("N", (8, 54, 70))
def test_kernel_equals_the_specification_bit_for_bit(N, K, clock):
    handle = handle_for(N)
    Tm, B = 6, 5
    for step, with_next in ((-1, True), (2, True), (4, False)):
        case = cases.random_case(N, K, Tm, B, seed=100 * N + 10 * K + step + 2, clock=clock, step=step, with_next=with_next)
        want = cases.run_spec(case)
        dev, host = run_device(handle, case), run_host(handle, case)
        check(case, want, dev, ("device", N, K, clock, step))
        check(case, want, host, ("host", N, K, clock, step))
    if clock:
        assert (want["gprice"] == case["gprice"]).all()   # the last step has no next adjoints: no price is touched
    assert want["gx"].any() and not want["gcap_carry"].any()


def test_hand_cases_on_the_device():
    case, want = cases.hand_case()
    handle = handle_for(4)
    for got in (run_device(handle, case), run_host(handle, case)):
        assert same_bits(got["gcap_carry"], want["gcap_carry"])
        assert same_bits(got["gx"][:, :, 0].copy(), want["gx0"]) and not got["gx"][:, :, 1:].any()
        assert same_bits(got["garr"], want["garr"])
        assert same_bits(got["gprice"], want["gprice"])


@pytest.mark.parametrize("N", (54, 70))
def test_every_copy_of_a_problem_gets_the_same_bits(N):
    import torch

    n = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 3
    one = cases.random_case(N, 2, 6, 1, seed=5, clock=True, step=2)
    rep = lambda a: None if a is None else np.repeat(a, n, axis=0)
    A1 = len(one["plan"]["a_evse"])
    assert A1 >= 1
    plan = dict(one["plan"], a_seg=(np.arange(n + 1) * A1).astype(np.int32), a_rate_seg=np.r_[np.tile(one["plan"]["a_rate_seg"][:-1], n),
                                                                                           one["plan"]["a_rate_seg"][-1:]].astype(np.int32))
    for k in ("a_evse", "a_slot", "a_len", "a_cap"):
        plan[k] = np.tile(one["plan"][k], n)
    case = dict(cur={k: rep(v) for k, v in one["cur"].items()}, applied=rep(one["applied"]), status=rep(one["status"]), x=rep(one["x"]),
                max_pilot=one["max_pilot"], plan=plan, cost=one["cost"], gdir=rep(one["gdir"]), nxt={k: rep(v) for k, v in one["nxt"].items()},
                garr=np.tile(one["garr"], n), gprice=rep(one["gprice"]))
    want = cases.run_spec(one)
    got = run_device(handle_for(N), case)
    for b in (0, 1, n // 2, n - 1):
        assert same_bits(got["gx"][b], want["gx"][0]) and same_bits(got["gcap_carry"][b], want["gcap_carry"][0]), b
        assert same_bits(got["gprice"][b], want["gprice"][0]) and same_bits(got["garr"][b * A1:(b + 1) * A1], want["garr"]), b
    assert all(same_bits(got["gx"][b], got["gx"][0]) and same_bits(got["gprice"][b], got["gprice"][0]) for b in range(n))


def test_refusals_leave_the_outputs_untouched():
    import copy

    import torch

    case, _ = cases.hand_case()
    handle = handle_for(4)
    infra = sites.balanced_three_phase(4, pods=1, load_fraction=0.35)
    flat = backend.SiteHandle(make_site(infra, "SOC", with_flat=True), 0)
    stream = torch.cuda.current_stream().cuda_stream

    def attempt(h, why, mutate):
        cur, plan, carry, kw = device_args(h, case)
        for k in ("garr", "gprice"):
            kw[k].fill_(7.5)
        cur, plan, kw = mutate(cur, plan, kw)
        with pytest.raises(ValueError, match=why):
            h.advance_vjp_device(cur, plan, case["plan"]["step"], carry, stream=stream, **kw)
        torch.cuda.synchronize()
        for t in (carry, kw["gx"], kw["garr"], kw["gprice"]):
            assert t is None or (t == 7.5).all().item(), why

    def no_x(cur, plan, kw):
        cur = copy.copy(cur)
        cur.x = None
        return cur, plan, kw

    def no_cost(cur, plan, kw):
        import dataclasses

        return cur, dataclasses.replace(plan, c_coef=None, c_weight=None, c_series=None), kw

    attempt(flat, "load-flattening or demand-charge row", lambda c, p, k: (c, p, k))
    attempt(handle, "x is null at step 1", no_x)
    attempt(handle, "gprice is given without a clock cost", no_cost)
    attempt(handle, "horizon_next is null", lambda c, p, k: (c, p, dict(k, horizon_next=None)))
    attempt(handle, "an output aliases an input .gx overlaps gq_next.", lambda c, p, k: (c, p, dict(k, gq_next=k["gx"])))
    flat.close()


# ---- the rollout ---------------------------------------------------------------------------------------------------------
def algorithm(iface, **options):
    alg = AdaptiveSchedulingAlgorithm(T.objective(), solver_options=options or None)
    alg.register_interface(iface)
    return alg


@functools.lru_cache(maxsize=None)
def taped():
    """(infra, table, result with its tape) of the CPU test's shape at tight tolerances"""
    infra, iface, fleets = T.setup()
    table = T.make_table(infra, iface, fleets)
    return infra, iface, table, algorithm(iface, **TIGHT).simulate_batch(table, T.STEPS, keep_tape=True)


def test_keep_tape_changes_no_bit():
    infra, iface, table, with_tape = taped()
    plain = algorithm(iface, **TIGHT).simulate_batch(table, T.STEPS)
    assert plain.tape is None and with_tape.tape is not None and len(with_tape.tape.states) == T.STEPS
    for k in ("pilots", "status", "flags", "iters"):
        assert same_bits(getattr(plain, k), getattr(with_tape, k)), k
    assert np.isin(plain.status, (1, 5)).all() and not plain.flags.any() and plain.pilots.any()


def downloaded(table, result):
    """the device's tape in the layout of tests/rollout_vjp_spec.forward"""
    site = result.tape.handle.site
    out = []
    for s, st in enumerate(result.tape.states):
        state = {k: getattr(st, k).cpu().numpy() for k in ("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap")}
        out.append(dict(state=state, batch=RS.to_batch(site, state), x=st.x.cpu().numpy(), y=st.y.cpu().numpy(),
                        applied=result.tape.pilots[s].cpu().numpy(), status=st.status.cpu().numpy(), flags=result.tape.flags[s].cpu().numpy()))
    return out


def test_rollout_gradients_against_the_specification():
    infra, iface, table, result = taped()
    w = T.loss_weights()
    g = rollout_gradients(result, w)
    tape = downloaded(table, result)
    want = RS.backward(table, infra, tape, w)
    assert (g.info.cpu().numpy()[:, :, 0] == 0).all() and (want["info"][:, :, 0] == 0).all()
    assert np.array_equal(g.info.cpu().numpy()[:, :, 1], want["info"][:, :, 1])   # the same working sets: rows of the Schur system
    worst = 0.0
    for name, got, ref in (("prices", g.prices.cpu().numpy(), want["prices"]), ("garr", g.garr.cpu().numpy(), want["garr"]),
                           ("limits", g.limits.cpu().numpy(), want["limits"])):
        err = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
        worst = max(worst, err)
        print(f"[rollout vjp gpu] {name}: |kernel - spec|_inf / max(1, |spec|_inf) = {err:.3e} (|spec|_inf {np.abs(ref).max():.3e})")
        assert np.abs(ref).max() > 1e-3, name
    print(f"[rollout vjp gpu] worst {worst:.3e} (bound {E2E_TOL:.1e}); vjp residuals {g.res.cpu().numpy().max(axis=(0, 1))}")
    req, ref_req = g.requested, RS.requested_gradients(table, want["garr"])
    assert [r.shape for r in req] == [(len(f),) for f in table.fleets]
    assert all(np.allclose(a, b, rtol=0, atol=E2E_TOL * max(1.0, float(np.abs(b).max()))) for a, b in zip(req, ref_req))
    assert worst <= E2E_TOL


def test_simulate_prices_backward_is_the_sweep():
    import torch

    from adacharge_amd import simulate_prices
    from adacharge_amd.diff import check_last_backward

    infra, iface, table, result = taped()
    w = torch.from_numpy(T.loss_weights()).cuda()
    want = rollout_gradients(result, w).prices.cpu().numpy()
    prices = torch.from_numpy(table.c_series.copy()).cuda().requires_grad_(True)
    pilots = simulate_prices(algorithm(iface, **TIGHT), table, prices)
    assert tuple(pilots.shape) == (T.STEPS, T.B, T.N) and same_bits(pilots.detach().cpu().numpy(), result.pilots)
    pilots.mul(w).sum().backward()
    assert same_bits(prices.grad.cpu().numpy(), want) and np.abs(want).max() > 1e-3
    assert check_last_backward() == 0


def test_a_long_horizon_rollout_with_vjp_long():
    from adacharge_amd.acn import Interface

    infra, iface, fleets = T.setup()
    steps, t_max = 3, 48
    iface = Interface(dict(iface.data, prices=np.tile(T.tariff(), 5)[: steps + t_max]))
    alg = algorithm(iface, vjp_long=True)
    table = FleetTable(fleets, infra, iface, alg.objective, steps, t_max=t_max)
    res = alg.simulate_batch(table, steps, keep_tape=True)
    g = rollout_gradients(res, np.random.default_rng(1).standard_normal((steps, T.B, T.N)))
    assert (g.info.cpu().numpy()[:, :, 0] == 0).all()
    assert tuple(g.prices.shape) == (T.B, steps + t_max) and tuple(g.limits.shape) == (T.B, res.tape.handle.site.M)
    assert tuple(g.info.shape) == (steps, T.B, 4) and tuple(g.res.shape) == (steps, T.B, 2)
    assert [r.shape for r in g.requested] == [(len(f),) for f in fleets]
    assert g.prices.abs().max().item() > 0 and np.isfinite(g.prices.cpu().numpy()).all()
    with pytest.raises(ValueError, match="keep_tape=True.*t_max = 48"):
        algorithm(iface).simulate_batch(FleetTable(fleets, infra, iface, alg.objective, steps, t_max=t_max), steps, keep_tape=True)
