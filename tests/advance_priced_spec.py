"""The rules of acnqp_advance_priced_device (include/acn_qp.h, "time passes") with a clock cost: rule 6b and the rule 9 that
reads its q', in plain Python-float loops, one problem at a time.  Rules 1-8 and 10 are tests/advance_spec.py's, called as
they stand; rule 4's admission is restated here only to know the windows of the sessions admitted in this step.  The
kernel's CLOCK instantiations (adacharge_amd/csrc/acn_qp_advance.hpp) are held to this bit for bit.

``cost``: None (the plain advance) or a dict with ``coef`` (float), ``weight`` (N,) and ``series`` (B, P)."""
import numpy as np

from tests import advance_spec as spec


def plan_and_cost(table, step):
    """(plan, cost) of a ``rollout.FleetTable`` as the dicts this spec takes, for the advance after period ``step``"""
    p = table.plan
    d = {k: getattr(p, k) for k in p._ARRAYS}
    d.update(done_tol=p.done_tol, kw_per_amp=p.kw_per_amp, step=step, a_seg=p.a_seg[step + 1])
    cost = None if p.c_series is None else dict(coef=p.c_coef, weight=p.c_weight, series=p.c_series)
    return d, cost


def admitted_windows(b, cur, applied, status, plan):
    """{evse: length} of the sessions rule 4 admits for problem ``b`` (the last one admitted on an EVSE counts)."""
    N, Tm = cur["lb"][b].shape
    K = cur["s_off"].shape[1]
    before = spec.advance_one(b, cur, applied, status, None, None, dict(plan, a_seg=None))   # rules 1-3: the slots the arrivals meet
    noff, nlen = before["s_off"].copy(), before["s_len"].copy()
    fresh = {}
    seg = plan.get("a_seg")
    n_arr = 0 if plan.get("a_evse") is None else len(plan["a_evse"])
    n_rates = 0 if plan.get("a_min") is None else len(plan["a_min"])
    if seg is None or not n_arr:
        return fresh
    for r in range(max(int(seg[b]), 0), min(int(seg[b + 1]), n_arr)):
        i, k, ln = int(plan["a_evse"][r]), int(plan["a_slot"][r]), int(plan["a_len"][r])
        r0 = int(plan["a_rate_seg"][r])
        ok = 0 <= i < N and 0 <= k < K and 1 <= ln <= Tm and 0 <= r0 and r0 + ln <= n_rates
        if ok and nlen[k, i] != 0:
            ok = False
        if ok:
            for kk in range(K):
                if nlen[kk, i] > 0 and noff[kk, i] < ln:
                    ok = False
        if not ok:
            continue
        noff[k, i], nlen[k, i] = 0, ln
        fresh[i] = ln
    return fresh


def advance_one(b, cur, applied, status, x, y, plan, cost=None):
    """Rules 1-10 with 6b for problem ``b``; the arguments of ``advance_spec.advance_one`` and ``cost``."""
    if cost is None:
        return spec.advance_one(b, cur, applied, status, x, y, plan)
    out = spec.advance_one(b, cur, applied, status, x, y, dict(plan, warm_arrival_gain=0.0))   # rule 9's shift only
    N, Tm = out["q"].shape
    hz = int(out["horizon"])
    q = out["q"]
    # 6b: where the horizon has a row, one product, one product, one sum per entry of the new horizon
    if not out["flags"] & spec.NO_ROW:
        coef = float(cost["coef"])
        for i in range(N):
            w = float(cost["weight"][i])
            for t in range(hz):
                price = float(cost["series"][b][plan["step"] + 1 + t])
                q[i, t] = float(q[i, t]) + coef * (w * price)
    # 9: a session admitted in this step starts at -gain * q', the q' of 6b
    gain = float(plan.get("warm_arrival_gain", 0.0))
    if x is not None and gain != 0.0:
        for i, ln in admitted_windows(b, cur, applied, status, plan).items():
            for t in range(ln):
                out["warm_x"][i, t] = (-gain) * float(q[i, t])
    return out


def advance(cur, applied, status, x, y, plan, cost=None):
    """``advance_one`` for every problem, stacked as ``advance_spec.advance`` stacks them."""
    B = len(cur["lb"])
    outs = [advance_one(b, cur, applied, status, x, y, plan, cost) for b in range(B)]
    res = {}
    for key in outs[0]:
        vals = [o[key] for o in outs]
        if key in ("horizon", "flags"):
            res[key] = np.array(vals, dtype=np.int32)
        elif np.isscalar(vals[0]):
            res[key] = np.array(vals, dtype=np.float64)
        else:
            res[key] = np.stack(vals)
    return res
