"""ORACLE -- test infrastructure only.  Nothing under adacharge_amd/ may import it.

A plain fp64 certificate of ONE answer of the library: the KKT conditions of the problem include/acn_qp.h states,
evaluated on the library's outputs (schedule ``x``, site-row multipliers ``y``, objective ``obj``) and the problem
statement (``builder.ProblemBatch`` / ``SiteData``) alone.  numpy only; no solver state, no activity thresholds.

Problem certified: the caller's problem with the Tikhonov floor the kernels add to LP-like problems,
``pd_eff = polish_ref.effective_pdiag(pdiag, reg_rel, |q_b|_inf, max_t max(lb, ub), T_b, has_prox)``
(acn_qp_common.hpp::effective_pdiag: ``qnorm`` and ``ubmax`` over the whole padded problem -- padding adds zeros --,
``ub`` raised to ``lb`` where it is below, the problem's own horizon ``T_b``).

Multiplier conventions, confirmed against oracle/admm_ref.py and oracle/admm_port.c (``y2 = rho (zhat - z)`` of the
site-row splitting ``G x_t = z_t``, rescaled by the row equilibration to the row order and units of ``acnqp_site.G``):

  * LINEAR row ``j`` and the peak row: ``y = rho (zhat - min(zhat, limit)) >= 0``, non-zero only where the row is
    tight.  A period whose peak is ``+inf`` gets ``y = 0`` exactly.
  * SOC pair ``(j, j + M)``: ``(y_j, y_{j+M}) = rho (1 - limit / |zhat|)_+ zhat`` -- the outward normal of the disc at
    ``z = (a, b)``: ``lam (a, b) / |(a, b)|`` with ``lam >= 0``, non-zero only on the circle.
  * flat row (load flattening, objective ``1/2 lf (v'x_t)^2``): ``y = rho (zhat - zhat rho / (rho + lf)) = lf z``, i.e.
    ``y_t = lf v'x_t`` -- the gradient of the term.
  * max row (demand charge, objective ``dc max(max_t v'x_t, dfloor)``): ``y_t = rho (zhat_t - min(zhat_t, level))``
    with the level of the prox: ``y_t >= 0``, non-zero only where ``v'x_t`` is the maximum, ``sum_t y_t = dc`` when
    that maximum is above ``dfloor`` and ``<= dc`` at the floor -- a subgradient of the term.

With these, stationarity of every problem is ``0 in pd_eff x + q + G'y + N_X(x)``, ``X`` = the box and the energy rows
of the sessions (the per-session set the kernels project onto).  It is measured as the natural residual of the
projection map, ``|x - Proj_X(x - g)|_inf`` with ``g = pd_eff x + q + G'y``, relative to ``max(1, |q|_inf)``: zero
exactly at a KKT point, with no threshold on what counts as active.  (A schedule moved by ``d`` amperes inside its free
set raises it by ``pd_eff d``.)

``certify`` returns the residuals (each normalised as its constant below says); ``failures`` compares them with the
limits of a status.
"""
from __future__ import annotations

import numpy as np

from .polish_ref import effective_pdiag

# Tolerances, set once from the C twin (oracle/admm_port.c) at default options (eps_abs = eps_rel = 1e-8, reg_rel 0.06,
# Anderson columns 5) on the pools of tests/test_kkt_certificate.py: 10x the worst value the twin reaches there.
PRI_TOL = 1.5e-6   # site rows: violation / max(1, limit).                          twin worst: 1.43e-7
STAT_TOL = 1.7e-7  # natural residual / max(1, |q|_inf).                            twin worst: 1.65e-8
COMP_TOL = 1.2e-6  # y slack / (max(1, |q|_inf) max(1, limit)); sign, cone           twin worst: 1.20e-7
                   # alignment, flat-row and +inf-peak multipliers / max(1, |q|_inf); |sum y_max - dc| / max(1, dc)
                   # (the worst site-row and multiplier values come from the load-flattening pool; the snapshot pools
                   #  reach 6.9e-8, 1.65e-8 and 6.2e-8)
EXACT_REL = 1e-12  # energy rows, reported objective and dead periods of y: roundoff only
INACCURATE_FACTOR = 1e3   # SOLVED_INACCURATE: the three tolerances above x 1e3

ST_SOLVED, ST_MAX_ITER, ST_SOLVED_INACCURATE = 1, 2, 5

# residual -> which limit applies
_KIND = dict(box="exact", zero="exact", finite="exact", energy="rel", obj="rel", y_dead="rel", site="pri", stat="stat",
             comp="comp", dual="comp", cone="comp", flat="comp", max_sum="comp")
_MAX_ITER_CHECKS = ("box", "zero", "finite")


def _sessions(batch, b):
    """(sid (N, Tm) int: session of each entry or -1, cap (S,)) of problem b"""
    N, Tm = batch.N, batch.Tm
    sid = np.full((N, Tm), -1, np.int64)
    caps = []
    for k in range(batch.K):
        for i in range(N):
            L = int(batch.s_len[b, k, i])
            if L > 0:
                o = int(batch.s_off[b, k, i])
                sid[i, o:o + L] = len(caps)
                caps.append(float(batch.s_cap[b, k, i]))
    return sid, np.asarray(caps, float)


def project_sessions(v, lb, ub, sid, cap, eq, iters=200):
    """Euclidean projection of v (N, Tm) onto {lb <= r <= ub, sum_{window s} r <= cap_s (== if eq)}: one scalar
    shift mu_s per session, found by vectorised bisection on the non-increasing sum_s clip(v - mu_s, lb, ub)."""
    S = len(cap)
    r = np.clip(v, lb, ub)
    if S == 0:
        return r
    on = sid >= 0
    s, vv, lo_b, hi_b = sid[on], v[on], lb[on], ub[on]
    ssum = lambda mu: np.bincount(s, np.clip(vv - mu[s], lo_b, hi_b), minlength=S)
    lo = np.full(S, np.inf)
    hi = np.full(S, -np.inf)
    np.minimum.at(lo, s, vv - hi_b)   # mu <= lo: every entry at ub
    np.maximum.at(hi, s, vv - lo_b)   # mu >= hi: every entry at lb
    lo = lo - 1.0
    hi = hi + 1.0
    if not eq:   # an inequality row binds only when the clipped point exceeds the cap
        lo = np.maximum(lo, 0.0)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        big = ssum(mid) > cap
        lo = np.where(big, mid, lo)
        hi = np.where(big, hi, mid)
    mu = 0.5 * (lo + hi)
    if not eq:
        mu = np.where(ssum(np.zeros(S)) <= cap, 0.0, mu)
    r[on] = np.clip(vv - mu[s], lo_b, hi_b)
    return r


def prox_terms(batch, b, x):
    """What SiteHandle._finish adds to the kernel's objective: 1/2 lf sum_t (v'x_t)^2 and dc max(max_t v'x_t, dfloor)"""
    site, out = batch.site, 0.0
    if site.has_flat:
        out += 0.5 * float(batch.lf[b]) * float(((site.G[site.flat_row] @ x) ** 2).sum())
    if site.has_max:
        out += float(batch.dc[b]) * max(float((site.G[site.max_row] @ x).max()), float(batch.dfloor[b]))
    return out


def certify(batch, b, x, y, obj, options=None):
    """Residuals of the answer (x (N, Tm), y (Mg, Tm), obj -- the objective as SiteHandle returns it, prox terms
    included) to problem ``b`` of ``batch``.  ``options``: the solver options (only ``reg_rel`` is read; default 0.06,
    acnqp_default_options).  Returns a dict name -> residual; compare with ``failures``."""
    site = batch.site
    x = np.asarray(x, float)
    y = np.asarray(y, float)
    N, Tm, Mg, M = site.N, batch.Tm, site.Mg, site.M
    T = int(batch.T[b])
    lb, q = batch.lb[b], batch.q[b]
    ub = np.maximum(batch.ub[b], lb)   # (the library raises ub to lb where it is below, aco.py:75)
    out = {}
    fin = bool(np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(obj))
    out["finite"] = 0.0 if fin else np.inf
    if not fin:
        return out
    reg_rel = 0.06 if options is None else float(options.reg_rel)
    qn = float(np.abs(q).max())
    has_prox = (site.has_flat and float(batch.lf[b]) > 0) or (site.has_max and batch.dc is not None and float(batch.dc[b]) > 0)
    pd_user = float(batch.pdiag[b])
    pd = effective_pdiag(pd_user, reg_rel, qn, float(ub.max()), T, has_prox)
    qs = max(1.0, qn)
    sid, cap = _sessions(batch, b)
    eq = bool(batch.s_eq[b])

    # ---- primal: box and exact zeros (the feasible iterate z), energy rows to roundoff --------------------------
    out["box"] = float(max(0.0, (lb - x).max(), (x - ub).max()))
    dead = (sid < 0)
    dead[:, T:] = True
    out["zero"] = float(np.abs(x[dead]).max()) if dead.any() else 0.0
    if len(cap):
        on = sid >= 0
        e = np.bincount(sid[on], x[on], minlength=len(cap))
        viol = np.abs(e - cap) if eq else np.maximum(e - cap, 0.0)
        out["energy"] = float((viol / np.maximum(1.0, np.abs(cap))).max())
    else:
        out["energy"] = 0.0

    # ---- site rows: values, slacks and the multiplier conditions, row by row in the order of G ------------------
    Gx = site.G @ x   # (Mg, Tm)
    lim = np.asarray(site.limits, float)
    site_v, comp, dual, cone = [0.0], [0.0], [0.0], [0.0]
    if M:
        if site.cone == 1:
            a, bb, ya, yb = Gx[:M], Gx[M:2 * M], y[:M], y[M:2 * M]
            nrm = np.hypot(a, bb)
            lam = np.hypot(ya, yb)
            sl = lim[:, None] - nrm
            scale = np.maximum(1.0, lim)[:, None]
            site_v.append(float((np.maximum(-sl, 0.0) / scale).max()))
            comp.append(float((lam * np.abs(sl) / scale).max()) / qs)
            safe = np.where(nrm > 0, nrm, 1.0)
            mis = np.where(nrm > 0, np.hypot(ya - lam * a / safe, yb - lam * bb / safe), 0.0)
            cone.append(float(mis.max()) / qs)
            r = 2 * M
        else:
            sl = lim[:, None] - Gx[:M]
            scale = np.maximum(1.0, lim)[:, None]
            site_v.append(float((np.maximum(-sl, 0.0) / scale).max()))
            comp.append(float((y[:M] * np.abs(sl) / scale).max()) / qs)
            dual.append(float(np.maximum(-y[:M], 0.0).max()) / qs)
            r = M
    else:
        r = 0
    flat = max_sum = 0.0
    if site.has_flat:
        flat = float(np.abs(y[r] - float(batch.lf[b]) * Gx[r]).max()) / qs
        r += 1
    if site.has_max:
        dc, dfl = float(batch.dc[b]), float(batch.dfloor[b])
        agg = Gx[r]
        top = float(agg.max())
        dual.append(float(np.maximum(-y[r], 0.0).max()) / qs)
        comp.append(float((y[r] * (top - agg)).max()) / (qs * max(1.0, abs(top))))
        ys = float(y[r].sum())
        max_sum = (abs(ys - dc) if top > dfl else max(ys - dc, 0.0)) / max(1.0, dc)
        r += 1
    if site.has_peak:
        pk = np.asarray(batch.peak[b], float)
        fin_pk = np.isfinite(pk)
        agg = Gx[r]
        if fin_pk.any():
            sl = pk[fin_pk] - agg[fin_pk]
            scale = np.maximum(1.0, np.abs(pk[fin_pk]))
            site_v.append(float((np.maximum(-sl, 0.0) / scale).max()))
            comp.append(float((y[r][fin_pk] * np.abs(sl) / scale).max()) / qs)
        dual.append(float(np.maximum(-y[r], 0.0).max()) / qs)
        if (~fin_pk).any():
            dual.append(float(np.abs(y[r][~fin_pk]).max()) / qs)
        r += 1
    out["site"] = max(site_v)
    out["comp"] = max(comp)
    out["dual"] = max(dual)
    out["cone"] = max(cone)
    out["flat"] = flat
    out["max_sum"] = max_sum
    ymax = float(np.abs(y).max()) if y.size else 0.0
    out["y_dead"] = (float(np.abs(y[:, T:]).max()) / ymax) if (ymax > 0 and T < Tm) else 0.0

    # ---- stationarity: natural residual of the projection map -------------------------------------------------
    g = pd * x + q + site.G.T @ y
    px = project_sessions(x - g, lb, ub, sid, cap, eq)
    out["stat"] = float(np.abs(x - px).max()) / qs

    # ---- the reported objective ----------------------------------------------------------------------------------
    terms = 0.5 * pd_user * x * x + q * x
    ref = float(terms.sum()) + prox_terms(batch, b, x)
    mag = float(np.abs(terms).sum()) + abs(prox_terms(batch, b, x))
    out["obj"] = abs(float(obj) - ref) / max(mag, 1e-300)
    return out


def limits(status):
    """name -> limit of every residual ``certify`` returns, for a problem of this status (ACNQP_STATUS_*)"""
    f = INACCURATE_FACTOR if status == ST_SOLVED_INACCURATE else 1.0
    tol = dict(exact=0.0, rel=EXACT_REL, pri=PRI_TOL * f, stat=STAT_TOL * f, comp=COMP_TOL * f)
    out = {k: tol[v] for k, v in _KIND.items()}
    if status not in (ST_SOLVED, ST_SOLVED_INACCURATE):   # MAX_ITER: box, exact zeros and written outputs only
        out = {k: out[k] for k in _MAX_ITER_CHECKS}
    return out


def failures(cert, status):
    """{name: (residual, limit)} of the residuals above their limit for this status; empty = certified"""
    return {k: (cert[k], lim) for k, lim in limits(status).items() if k in cert and not cert[k] <= lim}
