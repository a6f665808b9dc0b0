"""SPECIFICATION of the library's dual report (acnqp_duals_device / acnqp_duals_host, csrc/acn_qp_duals.hpp): numpy only,
test infrastructure only -- nothing under adacharge_amd/ may import it.

For problem ``b`` of a batch and an answer ``(x, y)`` (schedule (N, Tm), site-row multipliers (Mg, Tm) in the row order and
units of ``acnqp_site.G``), in the minimisation form of include/acn_qp.h:

    pd_eff = the diagonal the kernels use (effective_pdiag: the Tikhonov floor of LP-like problems included)
    g      = pd_eff x + q + G'y
    v      = x - g
    mu_s   = the shift with  sum_{t in window s} clip(v - mu_s, lb, ub) = cap_s        (``waterfill``)
    z      = -(g + mu_s) inside a window, 0 outside            (> 0: multiplier of ub, < 0: of lb)

and four residuals: ``stat = |x - clip(v - mu)|_inf``, ``energy``, ``site``, ``comp`` (oracle/kkt.py's scalings).

Every sum over a session window runs over its periods in increasing order, and ``G'y`` over the rows of G in increasing
order: the decisions that compare a sum of bounds with a cap (the tie rule) are then the same on every implementation.
"""
import numpy as np

ST_SOLVED, ST_SOLVED_INACCURATE = 1, 5
RES_NAMES = ("stat", "energy", "site", "comp")


def effective_pdiag(pd_user, reg_rel, qnorm, ubmax, horizon, has_prox):
    """acn_qp_common.hpp::effective_pdiag"""
    if has_prox or not ubmax > 0 or pd_user * ubmax > 1e-6 * qnorm:
        return pd_user
    return max(pd_user, reg_rel * qnorm / (ubmax * max(horizon, 1)))


def _seqsum(a):
    s = 0.0
    for e in a:
        s += float(e)
    return s


def waterfill(v, lb, ub, cap, eq):
    """The shift mu with sum_t clip(v_t - mu, lb_t, ub_t) = cap over one window (ub >= lb), exactly: the iteration ends on
    the linear segment of the piecewise-linear sum that holds the root and solves that segment's equation.

    Inequality row: 0 when sum clip(v) <= cap.  Where the admissible shifts form an interval (no entry strictly inside
    its bounds) the value of least magnitude is returned; a cap the bounds cannot reach counts as reached at the
    nearest end (all entries on ub / on lb).  Entries with lb == ub have no breakpoint."""
    L = len(v)
    v, lb, ub = (np.asarray(a, float) for a in (v, lb, ub))
    if not eq and _seqsum(np.minimum(np.maximum(v, lb), ub)) <= cap:
        return 0.0
    f_hi, f_lo = _seqsum(ub), _seqsum(lb)
    bmin, bmax = np.inf, -np.inf   # below bmin every entry is on ub, from bmax on every entry is on lb
    for t in range(L):
        if ub[t] > lb[t]:
            bmin = min(bmin, v[t] - ub[t])
            bmax = max(bmax, v[t] - lb[t])
    if cap >= f_hi:
        return min(0.0, bmin)
    if cap <= f_lo:
        return max(0.0, bmax)
    lo, hi = bmin, bmax   # sum(lo) = f_hi > cap > f_lo = sum(hi)
    m = 0.0 if lo < 0.0 < hi else 0.5 * (lo + hi)
    for _ in range(2 * L + 8):
        # the segment [below, above) that holds m: entries on ub, on lb, free
        sv = sb = 0.0
        nf = 0
        below, above = lo, hi
        for t in range(L):
            bu, bl = v[t] - ub[t], v[t] - lb[t]
            if ub[t] > lb[t]:
                for bp in (bu, bl):
                    if bp <= m:
                        below = max(below, bp)
                    else:
                        above = min(above, bp)
            if m < bu:
                sb += ub[t]
            elif m >= bl:
                sb += lb[t]
            else:
                sv += v[t]
                nf += 1
        if nf > 0:
            r = ((sv + sb) - cap) / nf
            if below <= r <= above:
                return r
            up = r > above
        else:
            d = sb - cap
            if d == 0.0:
                return min(max(0.0, below), above)
            up = d > 0.0
            r = np.nan
        if up:
            lo = above
        else:
            hi = below
        m = r if (nf > 0 and lo < r < hi) else 0.5 * (lo + hi)
        if not lo < m < hi:
            return lo
    return m


def duals(batch, b, x, y, status=ST_SOLVED, reg_rel=0.06):
    """dict(mu (K, N), z (N, Tm), res (4,) = stat, energy, site, comp, plus g, pd, qn) of the answer (x, y) to problem b"""
    site = batch.site
    N, Tm, K, M, Mg = site.N, batch.Tm, batch.K, site.M, site.Mg
    mu = np.zeros((K, N))
    z = np.zeros((N, Tm))
    if int(status) not in (ST_SOLVED, ST_SOLVED_INACCURATE):
        return dict(mu=mu, z=z, res=np.full(4, np.inf))
    x = np.asarray(x, float)
    y = np.asarray(y, float).reshape(Mg, Tm)
    T = int(batch.T[b])
    lb, q = batch.lb[b], batch.q[b]
    ub = np.maximum(batch.ub[b], lb)
    qn = float(np.abs(q).max())
    qs = max(1.0, qn)
    has_prox = bool((site.has_flat and float(batch.lf[b]) > 0) or (site.has_max and float(batch.dc[b]) > 0))
    pd = effective_pdiag(float(batch.pdiag[b]), reg_rel, qn, float(ub.max()), T, has_prox)
    gty = np.zeros((N, Tm))
    for j in range(Mg):   # rows in order
        gty += site.G[j][:, None] * y[j][None, :]
    g = pd * x + q + gty
    v = x - g
    px = np.minimum(np.maximum(v, lb), ub)   # outside every window: the box alone
    eq = bool(batch.s_eq[b])
    energy = 0.0
    for k in range(K):
        for i in range(N):
            o, L = int(batch.s_off[b, k, i]), int(batch.s_len[b, k, i])
            o2 = min(o + L, Tm)
            if L <= 0 or o2 <= o:
                continue
            cap = float(batch.s_cap[b, k, i])
            w = slice(o, o2)
            m = waterfill(v[i, w], lb[i, w], ub[i, w], cap, eq)
            mu[k, i] = m
            px[i, w] = np.minimum(np.maximum(v[i, w] - m, lb[i, w]), ub[i, w])
            z[i, w] = -(g[i, w] + m)
            e = _seqsum(x[i, w])
            viol = abs(e - cap) if eq else max(e - cap, 0.0)
            energy = max(energy, viol / max(1.0, abs(cap)))
    z[:, T:] = 0.0
    stat = float(np.abs(x - px).max())

    # site rows: violation and multiplier x slack, oracle/kkt.py's scalings
    Gx = np.zeros((Mg, Tm))
    for i in range(N):
        Gx += site.G[:, i][:, None] * x[i][None, :]
    lim = np.asarray(site.limits, float)
    sv, comp = 0.0, 0.0
    if M:
        scale = np.maximum(1.0, lim)[:, None]
        if site.cone == 1:
            sl = lim[:, None] - np.hypot(Gx[:M], Gx[M:2 * M])
            lam = np.hypot(y[:M], y[M:2 * M])
        else:
            sl = lim[:, None] - Gx[:M]
            lam = y[:M]
        sv = max(sv, float((np.maximum(-sl, 0.0) / scale).max()))
        comp = max(comp, float((lam * np.abs(sl) / scale).max()) / qs)
    if site.has_max:
        agg = Gx[site.max_row]
        top = float(agg.max())
        comp = max(comp, float((y[site.max_row] * (top - agg)).max()) / (qs * max(1.0, abs(top))))
    if site.has_peak:
        pk = np.asarray(batch.peak[b], float)
        fin = np.isfinite(pk)
        if fin.any():
            sl = pk[fin] - Gx[Mg - 1][fin]
            scale = np.maximum(1.0, np.abs(pk[fin]))
            sv = max(sv, float((np.maximum(-sl, 0.0) / scale).max()))
            comp = max(comp, float((y[Mg - 1][fin] * np.abs(sl) / scale).max()) / qs)
    return dict(mu=mu, z=z, res=np.array([stat, energy, sv, comp]), g=g, pd=pd, qn=qn)


def duals_batch(batch, x, y, status=None, reg_rel=0.06):
    """(mu (B, K, N), z (B, N, Tm), res (B, 4)) of a whole batch"""
    out = [duals(batch, b, x[b], y[b], ST_SOLVED if status is None else status[b], reg_rel) for b in range(batch.B)]
    return np.stack([o["mu"] for o in out]), np.stack([o["z"] for o in out]), np.stack([o["res"] for o in out])
