"""The four rules of acnqp_prepare_device (include/acn_qp.h, "before the solve") in plain Python loops, one problem at a
time.  This is the yardstick: the kernel (adacharge_amd/csrc/acn_qp_prepare.hpp) is held to it bit for bit.  Everything is a
copy or a comparison except the row test of rule 2: IEEE-754 doubles (Python floats: the arithmetic of numpy float64 scalars,
one rounding per product and per sum, never fused), sums over increasing i, squares compared (no square root, no hypot)."""
import math

import numpy as np

SLACK = 1e-7    # utils.py:5-12
FUTURE = 1      # flag: a live slot with s_off > 0


def order_of(s_off, s_len, key):
    """Rule 1 and the positions of rule 3 for one problem: the live slots in ascending (key, i), then the EVSEs without a
    live slot in increasing i."""
    N = len(s_len)
    live = [i for i in range(N) if s_len[i] > 0]
    live.sort(key=lambda i: (int(key[i]), i))
    return live + [i for i in range(N) if not s_len[i] > 0]


def prepare_one(b, cur, key, cre, cim, limits, min_pilot, lb, ub):
    """Rules 1-4 for problem ``b``; ``lb`` / ``ub`` (B, N, Tm) are changed in place.  Returns
    ``(v_evse, v_arrived, v_cap, flag, margin, accepted)``: ``margin`` the smallest distance in amperes of a decision of
    rule 2 from its threshold (``s_cap - want``; ``limit + 1e-7 - magnitude`` of a row -- for a visit the network refused,
    the LARGEST such distance among the rows that refused it, since all of them would have to flip), ``accepted`` (N,)
    1 accepted, 0 refused by the network, -1 refused by the cap, -2 not visited."""
    s_off, s_len, s_cap = (np.asarray(cur[k]).reshape(lb.shape[0], -1)[b] for k in ("s_off", "s_len", "s_cap"))
    N = lb.shape[1]
    M = 0 if cre is None else cre.shape[0]
    order = order_of(s_off, s_len, key[b])
    present = [bool(s_len[i] > 0 and s_off[i] == 0) for i in range(N)]
    flag = FUTURE if any(s_len[i] > 0 and s_off[i] > 0 for i in range(N)) else 0
    margin = np.inf
    accepted = np.full(N, -2, dtype=np.int64)
    if min_pilot is not None:
        lim = [float(limits[j]) + SLACK for j in range(M)]
        lim2 = [lim[j] * lim[j] for j in range(M)]
        cr, ci = (cre.tolist(), cim.tolist()) if M else ([], [])
        w = [0.0] * N
        for i in order:
            if not present[i]:
                continue
            want = float(min_pilot[i])
            w[i] = want
            ok_cap = bool(s_cap[i] >= want)
            margin = min(margin, abs(float(s_cap[i] - want)))
            ok_rows, d_ok, d_bad = True, np.inf, 0.0
            for j in range(M):
                re, im, rj, ij = 0.0, 0.0, cr[j], ci[j]
                for k in range(N):
                    pa = rj[k] * w[k]
                    pb = ij[k] * w[k]
                    re = re + pa
                    im = im + pb
                mag2 = re * re + im * im
                d = abs(math.sqrt(mag2) - lim[j])       # (the margin only: no decision reads a square root)
                if mag2 <= lim2[j]:
                    d_ok = min(d_ok, d)
                else:
                    ok_rows = False
                    d_bad = max(d_bad, d)
            if ok_cap:                                       # (a cap refusal does not depend on the network's sums)
                margin = min(margin, d_ok if ok_rows else d_bad)
            if ok_cap and ok_rows:
                accepted[i] = 1
                l0 = lb[b, i, 0]
                lo = l0 if l0 > want else want
                u0 = ub[b, i, 0]
                lb[b, i, 0] = lo
                ub[b, i, 0] = lo if u0 < lo else u0
            else:
                accepted[i] = 0 if ok_cap else -1
                w[i] = 0.0
                lb[b, i, 0] = 0.0
                ub[b, i, 0] = 0.0
    v_evse = np.array(order, dtype=np.int32)
    v_arrived = np.array([1 if present[i] else 0 for i in order], dtype=np.uint8)
    v_cap = np.array([(s_cap[i] if s_cap[i] <= ub[b, i, 0] else ub[b, i, 0]) if present[i] else 0.0 for i in order], dtype=np.float64)
    return v_evse, v_arrived, v_cap, flag, margin, accepted


def prepare(cur, key, cre, cim, limits, min_pilot):
    """The whole batch: ``cur`` a dict with lb, ub (B, N, Tm) and s_off, s_len, s_cap (B, 1, N) or (B, N); ``key`` (B, N).
    Returns a dict: lb, ub (copies), v_evse, v_arrived, v_cap (B, N), flags (B,), margin (B,), accepted (B, N)."""
    lb, ub = np.array(cur["lb"], np.float64), np.array(cur["ub"], np.float64)
    B, N, _ = lb.shape
    out = dict(lb=lb, ub=ub, v_evse=np.empty((B, N), np.int32), v_arrived=np.empty((B, N), np.uint8), v_cap=np.empty((B, N)),
               flags=np.empty(B, np.int32), margin=np.empty(B), accepted=np.empty((B, N), np.int64))
    for b in range(B):
        ve, va, vc, fl, mg, acc = prepare_one(b, cur, key, cre, cim, limits, min_pilot, lb, ub)
        out["v_evse"][b], out["v_arrived"][b], out["v_cap"][b], out["flags"][b], out["margin"][b], out["accepted"][b] = ve, va, vc, fl, mg, acc
    return out
