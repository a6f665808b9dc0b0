"""The six rules of acnqp_estimate_device (include/acn_qp.h, "the ramp-down estimator") in plain Python loops, one EVSE at
a time.  This is the yardstick: the kernel (adacharge_amd/csrc/acn_qp_estimate.hpp) is held to it bit for bit, and so is
``adacharge_amd.SimpleRampdown``, the host-side estimator.  Every floating-point operation here is one IEEE-754 double
operation on Python floats: comparisons, at most two subtractions and one addition per EVSE.

The estimator is acnportal's ``SimpleRampdown`` (acnportal.algorithms.upper_bound_estimator), AS RECALLED -- acnportal is not
installed here, so THIS FILE IS THE DEFINITION:
  * a session seen for the first time gets its own ``max_rates[0]`` as its bound
  * a session that drew more than ``down_threshold`` less than its pilot has the bound set to what it drew plus
    ``up_increment``
  * otherwise a session that drew within ``up_threshold`` of its bound has the bound raised by ``up_increment``
and the reference (ada.py:143-146) caps the session's ``max_rates`` with the bound, then ``reconcile_max_and_min`` with
``choose_min=True``.  Units are the slot state's: amperes."""
import math

import numpy as np

SOLVED, SOLVED_INACCURATE = 1, 5
BAD_FRESH, BAD_SLOT = 1, 2


def ramp(u, pp, pr, up_threshold, down_threshold, up_increment):
    """the arithmetic of rule 4: the bound ``u`` after ``pp`` was offered and ``pr`` drawn"""
    if pp - pr > down_threshold:
        return pr + up_increment
    if u - pr < up_threshold:
        return u + up_increment
    return u


def estimate_one(Tm, s_off, s_len, lb, ub, fresh, est, pilot, actual, served, up_threshold, down_threshold, up_increment):
    """Rules 1-5 for one EVSE: (est', ub_out (Tm,), flag bits).  ``lb``, ``ub``: its (Tm,) rows; ``pilot``: what it was offered
    in the period before, or None (no history); ``actual``: what it drew, or None (what is offered is drawn); ``served``: the
    status of its problem is accepted."""
    flags = 0
    ln = int(s_len)
    out = [float(v) for v in ub]
    # 1 slot
    if ln > Tm:
        flags |= BAD_SLOT
    present = ln > 0 and int(s_off) == 0 and ln <= Tm
    if not present:
        # 2 absent
        if int(fresh) != 0:
            flags |= BAD_FRESH
        return math.inf, np.array(out), flags
    if int(fresh) != 0:
        # 3 first sight
        u = float(ub[0])
    else:
        # 4 update
        u = float(est)
        if pilot is not None:
            pp = float(pilot) if served and float(pilot) > 0.0 else 0.0
            pr = pp if actual is None else (float(actual) if served else 0.0)
            u = ramp(u, pp, pr, float(up_threshold), float(down_threshold), float(up_increment))
    # 5 output
    for t in range(ln):
        v = u if u < out[t] else out[t]
        lo = float(lb[t])
        out[t] = lo if v < lo else v
    return u, np.array(out), flags


def estimate(cur, fresh, pilots, actual, status, up_threshold, down_threshold, up_increment, est):
    """Rules 1-6 for a batch.  ``cur``: dict with s_off, s_len (B, 1, N) or (B, N) and lb, ub (B, N, Tm); ``fresh`` (B, N) int32;
    ``pilots``, ``actual`` (B, N) or None; ``status`` (B,) or None; ``est`` (B, N).  Returns a dict of est (B, N), ub (B, N, Tm)
    -- the capped bounds -- and flags (B,) int32; nothing given is changed."""
    B, N, Tm = np.shape(cur["ub"])
    if actual is not None and pilots is None:
        raise ValueError("actual is given without pilots")
    off, ln = np.reshape(cur["s_off"], (B, N)), np.reshape(cur["s_len"], (B, N))
    nest, nub = np.empty((B, N)), np.empty((B, N, Tm))
    flags = np.zeros(B, np.int32)
    for b in range(B):
        served = status is None or int(status[b]) in (SOLVED, SOLVED_INACCURATE)
        for i in range(N):
            nest[b, i], nub[b, i], f = estimate_one(Tm, off[b, i], ln[b, i], cur["lb"][b, i], cur["ub"][b, i], fresh[b, i], est[b, i],
                                                    None if pilots is None else pilots[b, i], None if actual is None else actual[b, i],
                                                    served, up_threshold, down_threshold, up_increment)
            flags[b] |= f
    return dict(est=nest, ub=nub, flags=flags)
