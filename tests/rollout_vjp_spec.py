"""A numpy closed loop and its backward sweep: the specification of ``rollout.simulate(..., keep_tape=True)`` and
``rollout.rollout_gradients``.  Test infrastructure: nothing under adacharge_amd/ imports it.

Forward, per step: tests/advance_priced_spec.advance -> a certified solve of every problem (oracle/polish_ref from the
point of oracle/ipm.py, or from a given point) -> tests/pilots_spec.continuous.  Backward: tests/advance_vjp_spec.py and
tests/vjp_spec.vjp in the order of the sweep, steps - 1 ... 0 and the last call at step -1."""
import numpy as np
import scipy.sparse as sp

from adacharge_amd.builder import ProblemBatch, make_site
from oracle.ipm import solve_conic_qp
from oracle.polish_ref import effective_pdiag, polish_batch_problem
from tests import advance_priced_spec as priced
from tests import advance_spec
from tests import advance_vjp_spec as AV
from tests import pilots_spec
from tests import vjp_spec as VS

REG_REL = 0.06   # acnqp_default_options


def to_batch(site, state):
    """the ``ProblemBatch`` of a state of tests/advance_spec.py (no peak, flat or max row)"""
    B, N, Tm = state["lb"].shape
    return ProblemBatch(site=site, B=B, Tm=Tm, K=state["s_off"].shape[1], T=np.asarray(state["horizon"], np.int32), lb=state["lb"],
                        ub=state["ub"], q=state["q"], pdiag=np.asarray(state["pdiag"], float), lf=np.zeros(B), s_off=state["s_off"],
                        s_len=state["s_len"], s_cap=state["s_cap"], s_eq=np.zeros(B, np.uint8), peak=None)


def ipm_point(batch, b):
    """(x (N, Tm), y (Mg, Tm)) of problem ``b`` by the interior-point oracle, in the units of the C ABI.  Variables whose
    bounds coincide are fixed (they must sit at 0: a rollout without minimum rates)."""
    site = batch.site
    N, Tm, T, M = site.N, batch.Tm, int(batch.T[b]), int(site.M)
    lb, ub = batch.lb[b][:, :T], np.maximum(batch.ub[b][:, :T], batch.lb[b][:, :T])
    q = batch.q[b][:, :T]
    x, y = np.zeros((N, Tm)), np.zeros((site.Mg, Tm))
    x[:, :T] = lb
    free = np.argwhere(ub > lb)
    if not len(free):
        return x, y
    assert not lb[ub <= lb].any()
    col = {(int(i), int(t)): c for c, (i, t) in enumerate(free)}
    n = len(free)
    pd = effective_pdiag(float(batch.pdiag[b]), REG_REL, float(np.abs(q).max()), float(ub.max()), T)
    rows, h = [], []

    def row(entries, rhs):
        r = np.zeros(n)
        for c, v in entries:
            r[c] += v
        rows.append(r)
        h.append(rhs)

    for (i, t), c in col.items():
        row([(c, 1.0)], ub[i, t])
        row([(c, -1.0)], -lb[i, t])
    for k in range(batch.K):
        for i in range(N):
            o, L = int(batch.s_off[b, k, i]), int(batch.s_len[b, k, i])
            if L:
                row([(col[i, t], 1.0) for t in range(o, o + L) if (i, t) in col], float(batch.s_cap[b, k, i]))
    G = np.asarray(site.G, float)
    soc = int(site.cone) == 1
    if not soc:
        for j in range(M):
            for t in range(T):
                row([(col[i, t], G[j, i]) for i in range(N) if (i, t) in col], float(site.limits[j]))
    l = len(rows)
    nq = 0
    if soc:
        for j in range(M):
            for t in range(T):
                row([], float(site.limits[j]))
                row([(col[i, t], -G[j, i]) for i in range(N) if (i, t) in col], 0.0)
                row([(col[i, t], -G[j + M, i]) for i in range(N) if (i, t) in col], 0.0)
                nq += 1
    qv = np.array([q[i, t] for i, t in free])
    res, (_, z, _) = solve_conic_qp(pd * sp.identity(n, format="csr"), qv, sp.csr_matrix(np.array(rows)), np.array(h), l, nq, tol=1e-9)
    assert res.status in ("optimal", "optimal_inaccurate"), res.status
    for (i, t), c in col.items():
        x[i, t] = res.x[c]
    if soc:
        zc = z[l:].reshape(M, T, 3)
        y[:M, :T], y[M:2 * M, :T] = -zc[:, :, 1], -zc[:, :, 2]
    else:
        y[:M, :T] = z[l - M * T: l].reshape(M, T)
    return x, y


def certified(batch, b, start=None):
    """(x (N, Tm), y (Mg, Tm)): a KKT point of problem ``b`` by the polish's specification, from ``start`` or the IPM's point"""
    x0, y0 = ipm_point(batch, b) if start is None else start
    T = int(batch.T[b])
    x, y = np.zeros_like(x0), np.zeros_like(y0)
    if not (batch.s_len[b] > 0).any():
        return x, y
    xp, info = polish_batch_problem(batch, b, x0, y0)
    assert info["ok"], (b, info["why"])
    x[:, :T], y[:, :T] = xp, info["y"]
    return x, y


def forward(table, infra, constraint_type="SOC", start=None):
    """The closed loop of ``table`` (a ``rollout.FleetTable`` with a clock cost or without).  Returns the tape: a list of
    dicts, one per step, with ``state`` (the arrays of tests/advance_spec.py), ``batch``, ``x``, ``y``, ``applied`` (B, N),
    ``status`` (B,), ``flags`` (B,) of the advance that built the state.  ``start``: the tape of another run, whose
    points start every polish (central differences stay on the base run's branch)."""
    site = make_site(infra, constraint_type)
    max_pilot = np.asarray(infra.max_pilot, float)[: table.N]
    B, N, Tm, K = table.B, table.N, table.Tm, table.K
    plan, cost = priced.plan_and_cost(table, -1)
    state = priced.advance(advance_spec.empty_state(B, N, Tm, K), np.zeros((B, N)), None, None, None, plan, cost)
    tape = []
    for s in range(table.steps):
        batch = to_batch(site, state)
        pts = [certified(batch, b, None if start is None else (start[s]["x"][b], start[s]["y"][b])) for b in range(B)]
        x, y = np.stack([p[0] for p in pts]), np.stack([p[1] for p in pts])
        applied = pilots_spec.continuous(x, max_pilot)[:, :, 0].copy()
        status = np.ones(B, np.int32)
        tape.append(dict(state=state, batch=batch, x=x, y=y, applied=applied, status=status, flags=state["flags"]))
        if s + 1 < table.steps:
            plan, cost = priced.plan_and_cost(table, s)
            state = priced.advance(state, applied, status, None, None, plan, cost)
    return tape


def backward(table, infra, tape, gdir, solve_vjp=None):
    """The sweep of ``rollout.rollout_gradients`` on a tape (of ``forward``, or one downloaded from the device with the
    same keys) for ``gdir`` (steps, B, N) = dL/d applied.  Returns dict(prices (B, P) or None, garr (A,), limits (B, M),
    info (steps, B, 4), res (steps, B, 2), steps: the per-step vjp results)."""
    max_pilot = np.asarray(infra.max_pilot, float)[: table.N]
    steps, B, N, Tm, K = table.steps, table.B, table.N, table.Tm, table.K
    M = int(tape[0]["batch"].site.M)
    garr = gprice = None
    limits = np.zeros((B, M))
    info, res = np.zeros((steps, B, 4), np.int32), np.zeros((steps, B, 2))
    nxt, per_step = None, [None] * steps
    empty = advance_spec.empty_state(B, N, Tm, K)
    for s in range(steps - 1, -2, -1):
        plan, cost = priced.plan_and_cost(table, -1)
        # the advance after period s took row s + 1 of the arrival segments; no advance follows the last step
        plan = dict(plan, step=s, t_max=Tm, a_seg=table.plan.a_seg[s + 1] if s + 1 < steps else None)
        if s >= 0:
            e = tape[s]
            out = AV.advance_vjp(e["state"], e["applied"], e["status"], e["x"], max_pilot, plan, cost, gdir[s], nxt, garr, gprice)
        else:
            out = AV.advance_vjp(empty, None, None, None, None, plan, cost, None, nxt, garr, gprice)
        garr, gprice = out["garr"], out["gprice"]
        if s < 0:
            break
        e = tape[s]
        vj = [VS.vjp(e["batch"], b, e["x"][b], e["y"][b], out["gx"][b], int(e["status"][b])) for b in range(B)]
        per_step[s] = vj
        gq, gcap = np.stack([v["gq"] for v in vj]), np.stack([v["gcap"] for v in vj])
        info[s], res[s] = np.stack([v["info"] for v in vj]), np.stack([v["res"] for v in vj])
        for b in range(B):
            limits[b] += vj[b]["grow"][:M].sum(axis=1)
        nxt = dict(gq=gq, gcap_vjp=gcap, gcap_carry=out["gcap_carry"], horizon=np.asarray(e["state"]["horizon"]), flags=np.asarray(e["flags"]))
    return dict(prices=gprice, garr=garr, limits=limits, info=info, res=res, steps=per_step)


def requested_gradients(table, garr):
    """per scenario, dL/d(requested kWh) of every fleet record: garr of the record the table made of it over its EVSE's
    kWh per A-period, 0 for a record never admitted"""
    out = [np.zeros(len(f)) for f in table.fleets]
    order = sorted(range(len(table._stays)), key=lambda j: (table._stays[j][2], table._stays[j][0]))
    for r, j in enumerate(order):
        b, i, _, _, n, _ = table._stays[j]
        out[b][n] = garr[r] / table.kwh_per_amp_period[i]
    return out
