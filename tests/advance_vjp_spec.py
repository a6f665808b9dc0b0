"""The rules A1 ... A7 of acnqp_advance_vjp_device (include/acn_qp.h, "the adjoint of time passes") in plain Python-float
loops, one problem at a time.  This is the yardstick: the kernel (adacharge_amd/csrc/acn_qp_advance_vjp.hpp) is held to it
bit for bit.  Every floating-point operation is one IEEE-754 double operation on Python floats, in the order written.

L is a scalar of the pilots ``applied`` (steps, B, N) as the advance saw them.  One call serves step ``plan["step"]``:
``cur`` holds the step's slot tables, ``applied / status / x`` what happened to it, ``gdir`` dL/d applied of the step, and
``nxt`` the adjoints of the state of the next step -- a dict with any of ``gq`` (B, N, Tm), ``gcap_vjp``, ``gcap_carry``
(B, K, N), ``horizon``, ``flags`` (B,); a missing entry (or ``nxt`` None) counts as zeros.  ``cost``: None or the dict of
tests/advance_priced_spec.py (``coef``, ``weight``; the series is not read).  ``plan``: the dict of tests/advance_spec.py."""
import numpy as np

from tests import advance_spec as spec


def replay_slots(b, cur, a, Tm, done_tol):
    """A3, rule 2: per slot (kept, served, off', len') with the forward's comparisons; ``a``: what rule 1 delivered"""
    K, N = cur["s_off"].shape[1:]
    kept, fed = np.zeros((K, N), bool), np.zeros((K, N), bool)
    noff, nlen = np.zeros((K, N), np.int32), np.zeros((K, N), np.int32)
    for k in range(K):
        for i in range(N):
            off, ln, cap = int(cur["s_off"][b, k, i]), int(cur["s_len"][b, k, i]), float(cur["s_cap"][b, k, i])
            if ln <= 0:
                continue
            if off < 0 or off >= Tm or off + ln > Tm:   # BAD_SLOT: retired unread
                continue
            if off > 0:
                off -= 1
            else:
                ln -= 1
                cap = cap - a[i]
                if cap < 0.0:
                    cap = 0.0
                fed[k, i] = True
            if ln == 0 or cap <= done_tol:
                fed[k, i] = False
                continue
            kept[k, i] = True
            noff[k, i], nlen[k, i] = off, ln
    return kept, fed, noff, nlen


def replay_arrivals(b, plan, noff, nlen, N, Tm):
    """A3, rule 4: [(record, slot k, evse i) admitted], [records refused]; ``noff, nlen`` are updated as the forward does"""
    K = noff.shape[0]
    admitted, refused = [], []
    seg = plan.get("a_seg")
    n_arr = 0 if plan.get("a_evse") is None else len(plan["a_evse"])
    n_rates = 0 if plan.get("a_min") is None else len(plan["a_min"])
    if seg is None or not n_arr:
        return admitted, refused
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
            refused.append(r)
            continue
        noff[k, i], nlen[k, i] = 0, ln
        admitted.append((r, k, i))
    return admitted, refused


def advance_vjp_one(b, cur, applied, status, x, max_pilot, plan, cost, gdir, nxt, garr, gprice):
    """A1 ... A7 for problem ``b``.  ``garr`` (A,) and ``gprice`` (B, P) or None are updated in place (the records of b's
    segment are written, the prices accumulated).  Returns (gx (N, Tm) or None at step -1, gcap_carry (K, N))."""
    K, N = cur["s_off"].shape[1:]
    step = int(plan["step"])
    first = step < 0
    nxt = nxt or {}
    Tm = int(plan["t_max"]) if "t_max" in plan else (x.shape[2] if x is not None else nxt["gq"].shape[2])
    # rule 1
    served = first or status is None or int(status[b]) in (spec.SOLVED, spec.SOLVED_INACCURATE)
    a = [float(applied[b][i]) if (not first and served) else 0.0 for i in range(N)]
    # A1
    G = [[0.0] * N for _ in range(K)]
    for k in range(K):
        for i in range(N):
            v = float(nxt["gcap_vjp"][b, k, i]) if nxt.get("gcap_vjp") is not None else 0.0
            c = float(nxt["gcap_carry"][b, k, i]) if nxt.get("gcap_carry") is not None else 0.0
            G[k][i] = v + c
    # A2
    if cost is not None and gprice is not None and nxt.get("gq") is not None:
        flags_next = int(nxt["flags"][b]) if nxt.get("flags") is not None else 0
        if not flags_next & spec.NO_ROW:
            hz = min(max(int(nxt["horizon"][b]), 0), Tm)
            coef = float(cost["coef"])
            for t in range(hz):
                acc = 0.0
                for i in range(N):
                    acc = acc + float(cost["weight"][i]) * float(nxt["gq"][b, i, t])
                gprice[b, step + 1 + t] = float(gprice[b, step + 1 + t]) + coef * acc
    # A3
    kept, fed, noff, nlen = replay_slots(b, cur, a, Tm, float(plan["done_tol"]))
    admitted, refused = replay_arrivals(b, plan, noff, nlen, N, Tm)
    # A4
    carry = np.zeros((K, N))
    for k in range(K):
        for i in range(N):
            carry[k, i] = G[k][i] if kept[k, i] else 0.0
    # A5, A6
    gx = None
    if not first:
        gx = np.zeros((N, Tm))
        for i in range(N):
            ga = float(gdir[b][i])
            for k in range(K):
                if kept[k, i] and fed[k, i] and served:
                    ga = ga - G[k][i]
            if not served:
                ga = 0.0
            x0 = float(x[b][i][0])
            gx[i, 0] = ga if (x0 >= 0.0 and x0 <= float(max_pilot[i])) else 0.0
    # A7
    for r, k, i in admitted:
        garr[r] = G[k][i]
    for r in refused:
        garr[r] = 0.0
    return gx, carry


def advance_vjp(cur, applied, status, x, max_pilot, plan, cost, gdir, nxt, garr=None, gprice=None):
    """``advance_vjp_one`` for every problem: dict(gx (B, N, Tm) or None, gcap_carry (B, K, N), garr (A,), gprice (B, P) or
    None).  ``garr`` / ``gprice``: the arrays of the previous call of a sweep (copied), or None for zeros."""
    B, K, N = cur["s_off"].shape
    n_arr = 0 if plan.get("a_evse") is None else len(plan["a_evse"])
    garr = np.zeros(n_arr) if garr is None else np.array(garr, dtype=np.float64)
    if cost is not None:
        P = int(cost["series_len"]) if "series_len" in cost else int(np.shape(cost["series"])[1])
        gprice = np.zeros((B, P)) if gprice is None else np.array(gprice, dtype=np.float64)
    outs = [advance_vjp_one(b, cur, applied, status, x, max_pilot, plan, cost, gdir, nxt, garr, gprice) for b in range(B)]
    gx = None if outs[0][0] is None else np.stack([o[0] for o in outs])
    return dict(gx=gx, gcap_carry=np.stack([o[1] for o in outs]), garr=garr, gprice=gprice if cost is not None else None)
