"""The ten rules of acnqp_advance_device (include/acn_qp.h, "time passes") in plain Python loops, one problem at a time.
This is the yardstick: the kernel (adacharge_amd/csrc/acn_qp_advance.hpp) is held to it bit for bit.  Every floating-point
operation here is one IEEE-754 double operation on Python floats: one subtraction per served slot, one ordered sum, one
product and comparisons."""
import numpy as np

SOLVED, SOLVED_INACCURATE = 1, 5
REFUSED, NO_ROW, BAD_SLOT = 1, 2, 4


def empty_state(B, N, Tm, K, Mg=0, dfloor=0.0):
    """A state with no session at all (what step = -1 starts from)."""
    return dict(horizon=np.ones(B, np.int32), lb=np.zeros((B, N, Tm)), ub=np.zeros((B, N, Tm)), q=np.zeros((B, N, Tm)),
                pdiag=np.zeros(B), lf=np.zeros(B), dc=np.zeros(B), dfloor=np.full(B, float(dfloor)),
                s_off=np.zeros((B, K, N), np.int32), s_len=np.zeros((B, K, N), np.int32), s_cap=np.zeros((B, K, N)),
                peak=np.full((B, Tm), np.inf))


def advance_one(b, cur, applied, status, x, y, plan):
    """Rules 1-10 for problem ``b``.  ``cur``: dict of the batch's arrays (lb, ub (B, N, Tm); s_off, s_len, s_cap (B, K, N);
    dfloor (B,)); ``plan``: dict with q_table (H, N, Tm), h_scal (H, 3), h_row (Tm + 1,), done_tol, kw_per_amp, step,
    peak_series (B, P) or None, a_seg (B + 1,) or None, a_evse, a_slot, a_len, a_cap, a_rate_seg, a_min, a_max.  Returns a
    dict of the problem's next arrays and its flags."""
    lb, ub = cur["lb"][b], cur["ub"][b]
    N, Tm = lb.shape
    K = cur["s_off"].shape[1]
    flags = 0
    # 1
    served = status is None or int(status[b]) in (SOLVED, SOLVED_INACCURATE)
    a = [float(applied[b][i]) if served else 0.0 for i in range(N)]
    # 3 (the shift)
    nlb, nub = np.zeros((N, Tm)), np.zeros((N, Tm))
    for i in range(N):
        for t in range(Tm - 1):
            nlb[i, t] = lb[i, t + 1]
            nub[i, t] = ub[i, t + 1]
    # 2, and the rest of 3
    noff, nlen, ncap = np.zeros((K, N), np.int32), np.zeros((K, N), np.int32), np.zeros((K, N))
    for k in range(K):
        for i in range(N):
            off, ln, cap = int(cur["s_off"][b, k, i]), int(cur["s_len"][b, k, i]), float(cur["s_cap"][b, k, i])
            if ln <= 0:
                continue
            if off < 0 or off >= Tm or off + ln > Tm:
                flags |= BAD_SLOT
                continue
            if off > 0:
                off -= 1
            else:
                ln -= 1
                cap = cap - a[i]
                if cap < 0.0:
                    cap = 0.0
            if ln == 0 or cap <= plan["done_tol"]:
                for t in range(off, off + ln):
                    nlb[i, t] = 0.0
                    nub[i, t] = 0.0
                continue
            noff[k, i], nlen[k, i], ncap[k, i] = off, ln, cap
    # 4
    fresh = {}
    seg = plan.get("a_seg")
    n_arr = 0 if plan.get("a_evse") is None else len(plan["a_evse"])
    n_rates = 0 if plan.get("a_min") is None else len(plan["a_min"])
    if seg is not None and n_arr:
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
                flags |= REFUSED
                continue
            noff[k, i], nlen[k, i], ncap[k, i] = 0, ln, float(plan["a_cap"][r])
            fresh[i] = ln
            for t in range(ln):
                lo, hi = float(plan["a_min"][r0 + t]), float(plan["a_max"][r0 + t])
                nlb[i, t] = lo
                nub[i, t] = lo if hi < lo else hi
    # 5
    hz = 1
    for k in range(K):
        for i in range(N):
            if nlen[k, i] > 0:
                hz = max(hz, int(noff[k, i]) + int(nlen[k, i]))
    # 6
    row = int(plan["h_row"][hz])
    H = len(plan["q_table"])
    if row < 0 or row >= H:
        flags |= NO_ROW
        q, pdiag, lf, dc = np.zeros((N, Tm)), 0.0, 0.0, 0.0
    else:
        q = np.array(plan["q_table"][row], dtype=np.float64)
        pdiag, lf, dc = (float(v) for v in plan["h_scal"][row])
    # 7
    peak = np.full(Tm, np.inf)
    if plan.get("peak_series") is not None:
        for t in range(hz):
            peak[t] = plan["peak_series"][b][plan["step"] + 1 + t]
    # 8
    s = 0.0
    for i in range(N):
        s = s + a[i]
    kw = float(plan["kw_per_amp"]) * s
    old = float(cur["dfloor"][b]) if cur.get("dfloor") is not None else 0.0
    dfloor = kw if kw > old else old
    out = dict(horizon=hz, lb=nlb, ub=nub, q=q, pdiag=pdiag, lf=lf, dc=dc, dfloor=dfloor, s_off=noff, s_len=nlen, s_cap=ncap,
               peak=peak, flags=flags)
    # 9
    if x is not None:
        wx = np.zeros((N, Tm))
        wx[:, : Tm - 1] = x[b][:, 1:]
        gain = float(plan.get("warm_arrival_gain", 0.0))
        if gain != 0.0:
            for i, ln in fresh.items():
                for t in range(ln):
                    wx[i, t] = (-gain) * float(q[i, t])
        out["warm_x"] = wx
    if y is not None:
        wy = np.zeros(y[b].shape)
        wy[:, : Tm - 1] = y[b][:, 1:]
        out["warm_y"] = wy
    return out


def advance(cur, applied, status, x, y, plan):
    """``advance_one`` for every problem, stacked: dict of (B, ...) arrays, ``flags`` (B,) int32 included."""
    B = len(cur["lb"])
    outs = [advance_one(b, cur, applied, status, x, y, plan) for b in range(B)]
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
