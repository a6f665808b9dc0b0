"""The launch-order key in numpy: what order_keys_kernel (adacharge_amd/csrc/acn_qp_pipeline.hpp) computes on the device.

A problem's key measures CONGESTION: how much of the schedule that ignores the site rows the site rows reject.
  greedy schedule   every session charges at its upper bound from its first period until its energy cap is used up:
                    rem = cap; for t in the window: d = max(lb, min(ub, max(rem, 0))), rem -= d.  Zero outside the windows
                    and at t >= horizon[b].
  cell              a (site row, period) pair.  Its ratio is load / limit, in double precision:
                      box row (LINEAR)                 (G x0)_t / limit
                      disc pair (SOC rows j, j + M)    hypot((G x0)_{j,t}, (G x0)_{j+M,t}) / limit_j
                      peak row                         sum_i x0_{i,t} / peak_t   (+inf never overloads)
                    The load-flattening and demand-charge rows have no limit and are no cells.
  overloaded        ratio > 1 + 1e-9;  C = number of overloaded cells
  key               min(1023, 8 min(C, 127) + min(7, sessions // 8)),  sessions = session slots with s_len > 0
tests/test_order_key_spec.py holds it to hand-made cases, tests/test_order_key_gpu.py holds the kernel to it."""
import numpy as np

OVERLOAD = 1.0 + 1e-9
KEY_MAX = 1023


def greedy_schedule(lb, ub, s_off, s_len, s_cap, horizon):
    """x0 (B, N, Tm) of lb, ub (B, N, Tm), s_off, s_len, s_cap (B, K, N) and horizon (B,)"""
    lb, ub = np.asarray(lb, np.float64), np.asarray(ub, np.float64)
    s_off, s_len, s_cap = np.asarray(s_off, np.int64), np.asarray(s_len, np.int64), np.asarray(s_cap, np.float64)
    B, N, Tm = lb.shape
    hz = np.asarray(horizon, np.int64).reshape(B, 1)
    x0 = np.zeros((B, N, Tm))
    for k in range(s_off.shape[1]):
        rem = s_cap[:, k, :].copy()
        for t in range(Tm):
            inside = (s_len[:, k] > 0) & (t >= s_off[:, k]) & (t < s_off[:, k] + s_len[:, k]) & (t < hz)
            d = np.maximum(lb[:, :, t], np.minimum(ub[:, :, t], np.maximum(rem, 0.0)))
            x0[:, :, t] = np.where(inside, d, x0[:, :, t])
            rem = np.where(inside, rem - d, rem)
    return x0


def cell_ratios(site, x0, peak=None):
    """(B, cells, Tm): the ratio of every cell -- the M infrastructure rows (a SOC pair is one), then the peak row"""
    G, M = np.asarray(site.G, np.float64), site.M
    B, _, Tm = x0.shape
    load = np.einsum("ji,bit->bjt", G, x0)
    with np.errstate(divide="ignore", invalid="ignore"):
        lim = np.asarray(site.limits, np.float64).reshape(1, M, 1)
        rows = [(np.hypot(load[:, :M], load[:, M:2 * M]) if site.cone == 1 else load[:, :M]) / lim]
        if site.has_peak and peak is not None:
            rows.append((x0.sum(axis=1) / np.asarray(peak, np.float64).reshape(B, Tm))[:, None, :])
    return np.concatenate(rows, axis=1)


def sessions(s_len):
    s_len = np.asarray(s_len)
    return (s_len.reshape(s_len.shape[0], -1) > 0).sum(axis=1)


def key_of(C, n_sessions):
    return np.minimum(KEY_MAX, 8 * np.minimum(C, 127) + np.minimum(7, n_sessions // 8)).astype(np.int32)


def session_keys(batch):
    """the key of a shape beyond the kernel's LDS budget, and of ACNQP_ORDER_KEY=sessions"""
    return np.minimum(KEY_MAX, sessions(batch.s_len)).astype(np.int32)


def describe(batch):
    """(ratios (B, cells, Tm), C (B,), keys (B,) int32) of a ProblemBatch"""
    x0 = greedy_schedule(batch.lb, batch.ub, batch.s_off, batch.s_len, batch.s_cap, batch.T)
    ratios = cell_ratios(batch.site, x0, batch.peak)
    C = (ratios > OVERLOAD).sum(axis=(1, 2))
    return ratios, C, key_of(C, sessions(batch.s_len))


def order_keys(batch):
    return describe(batch)[2]


def margin(ratios):
    """distance of the closest cell ratio to 1: a test whose margin exceeds 1e-6 cannot be decided by rounding"""
    r = ratios[np.isfinite(ratios)]
    return float(np.abs(r - 1.0).min()) if r.size else np.inf
