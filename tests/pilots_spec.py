"""Specification of the pilot-signal kernel (adacharge_amd/csrc/acn_qp_pilots.hpp, acnqp_pilots_* in include/acn_qp.h)
in numpy with plain loops: one function per mode, for rates (B, N, Tm).  The kernel is held to these BIT FOR BIT; that
is possible because every operation below is an IEEE-754 double add, multiply or comparison in a stated order (numpy's
elementwise ``*`` and ``+`` round once each and never fuse).

Inputs are the arrays of ``acnqp_pilot_plan`` as ``postprocessing.pilot_plan_arrays`` makes them: ``levels`` (N, L) padded
with +inf, ``cre`` / ``cim`` (M, N), ``limits`` (M,), ``sess_seg`` (B + 1,), ``s_evse`` / ``s_arrived`` / ``s_cap`` (S,).
"""
import numpy as np

EPS = 0.05      # post.py:10-31
SLACK = 1e-7    # utils.py:5-12


def floor_to_set(x, levels):
    """post.py:10-31 as a count: pos = #{k : levels[k] < x + 0.05}; pos == 0 gives the first level, pos == L the last,
    otherwise level pos - 1 (one scalar, one EVSE's padded level row)."""
    xe = x + EPS
    pos = 0
    for k in range(len(levels)):
        if levels[k] < xe:
            pos += 1
    return levels[0] if pos == 0 else levels[pos - 1]


def continuous(x, max_pilot):
    """max(min(x, max_pilot_i), 0)."""
    out = np.empty_like(x)
    B, N, Tm = x.shape
    for b in range(B):
        for i in range(N):
            for t in range(Tm):
                v = x[b, i, t] if x[b, i, t] <= max_pilot[i] else max_pilot[i]
                out[b, i, t] = v if v >= 0.0 else 0.0
    return out


def discrete(x, levels):
    """max(floor_to_set(x, levels_i, 0.05), 0) on every entry, padding periods included.  (The count of one EVSE's row
    is taken for all its entries at once: comparisons only, so the vector form cannot differ from ``floor_to_set``.)"""
    B, N, Tm = x.shape
    out = np.empty_like(x)
    for i in range(N):
        xe = x[:, i, :] + EPS
        pos = np.zeros(xe.shape, dtype=np.int64)
        for k in range(levels.shape[1]):
            pos += levels[i, k] < xe
        v = levels[i][np.maximum(pos - 1, 0)]
        out[:, i, :] = np.where(v >= 0.0, v, 0.0)
    return out


def increment(cur, levels):
    """post.py:58-74: the next larger level, clipped at the last finite one."""
    last = levels[0]
    for k in range(len(levels)):
        if levels[k] < np.inf:
            last = levels[k]
    for k in range(len(levels)):
        if levels[k] > cur and levels[k] < np.inf:
            return levels[k]
    return last


def _seq_sum(v):
    s = 0.0
    for k in range(len(v)):
        s = s + v[k]
    return s


def reallocate(x, levels, cre, cim, limits, sess_seg, s_evse, s_arrived, s_cap):
    """DISCRETE everywhere, then the round robin of post.py:189-258 on period 0 of every problem.  Returns
    ``(pilots (B, N, Tm), visits (B,) int32, margin (B,))``: ``visits[b]`` the visits of an active EVSE made (each is an
    increment or a retirement, so a terminating input makes at most N L), -1 when the problem was still active after
    N L of them; ``margin[b]`` the smallest distance, in amperes, of a decision that depends on a summation order (the
    aggregate against the peak, a row magnitude against its limit) from its threshold -- for a refused trial the
    LARGEST such distance among the tests that refused it (all of them would have to flip), infinite when the cap
    refused it."""
    B, N, Tm = x.shape
    M, L = cre.shape[0], levels.shape[1]
    out = discrete(x, levels)
    visits = np.zeros(B, dtype=np.int32)
    margin = np.full(B, np.inf)
    lim = limits + SLACK
    lim2 = lim * lim
    for b in range(B):
        x0 = x[b, :, 0]
        col = out[b, :, 0].copy()
        peak = _seq_sum(x0)
        sess = list(range(int(sess_seg[b]), int(sess_seg[b + 1])))
        key = [-(x0[s_evse[s]] - col[s_evse[s]]) for s in sess]
        order = sorted(range(len(sess)), key=lambda k: (key[k], k))     # stable sort by the EVSE's rounding loss
        order = [int(s_evse[sess[k]]) for k in order]                   # ALL sessions: an EVSE may appear twice
        active = np.zeros(N, dtype=bool)
        cap = np.zeros(N)
        for s in sess:
            if s_arrived[s]:
                active[s_evse[s]] = True
                cap[s_evse[s]] = s_cap[s]
        n, p, bound = 0, 0, N * L
        while len(order) and active.any():
            if n == bound:          # still active after N L visits: the reference would never return
                n = -1
                break
            i = order[p % len(order)]
            p += 1
            if not active[i]:
                continue
            n += 1
            if col[i] >= cap[i]:
                active[i] = False
                continue
            nxt = increment(col[i], levels[i])
            trial = col.copy()
            trial[i] = nxt
            total = _seq_sum(trial)
            re, im = np.zeros(M), np.zeros(M)
            for k in range(N):       # increasing i; every product and every sum rounded once (all rows at a time)
                re = re + cre[:, k] * trial[k]
                im = im + cim[:, k] * trial[k]
            mag2 = re * re + im * im
            ok_peak, ok_cap, ok_rows = total <= peak, nxt <= cap[i], bool(np.all(mag2 <= lim2))
            d_peak = abs(total - peak)
            d_rows = np.abs(np.sqrt(mag2) - lim)      # (the margin only: no decision reads a square root)
            if ok_peak and ok_cap and ok_rows:
                col[i] = nxt
                margin[b] = min(margin[b], d_peak, d_rows.min() if M else np.inf)
            else:
                active[i] = False
                if ok_cap:
                    worst = max([d_peak] * (not ok_peak) + list(d_rows[mag2 > lim2]))
                    margin[b] = min(margin[b], worst)
        out[b, :, 0] = col
        visits[b] = n
    return out, visits, margin
