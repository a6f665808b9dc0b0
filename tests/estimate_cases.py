"""The shared cases of the estimator tests (tests/test_estimate_spec.py, tests/test_estimate_gpu.py): for every shape
(N, B, Tm) a few independent CALLS -- each a slot state (s_off, s_len, lb, ub), the fresh marks, the estimate so far and the
history (pilots, actual, status) -- built so that every branch of the six rules occurs in every shape, N = 1 and B = 1
included: an element is given one of sixteen situations in rotation, a problem in seven is handed a status that is not
accepted, one call in four has no ``actual`` (what is offered is drawn), one in eight no history at all, and a shape with
few elements gets more calls.  ``occurrences`` finds the branches again FROM THE DATA, not from the rotation, and
``check_occurrences`` asserts them: the CPU suite runs it for every shape.  At Tm = 1 two branches cannot occur (a cap
between the bounds of two periods, a window shorter than Tm) and are not asked for.

The thresholds are not the defaults, so that none equals another: all three are exact in binary, and so are the pilots of
the two situations that sit ON a threshold to the bit.  The sites are synthetic: the entries read nothing of a site but
its number of EVSEs."""
import functools
import math

import numpy as np

from tests import estimate_spec as spec

NS, BS, TMS = (1, 54, 64, 65, 130), (1, 3, 257), (1, 5, 12)
UP, DOWN, INC = 0.75, 1.5, 0.5       # up_threshold, down_threshold, up_increment
PARAMS = (UP, DOWN, INC)
N_SITUATIONS = 16


def _element(kind, rng, Tm):
    """one EVSE in situation ``kind``: (s_off, s_len, fresh, est, pilot, actual, lb (Tm,), ub (Tm,))"""
    off, ln, fresh, est = 0, int(rng.integers(1, Tm + 1)), 0, 32.0
    pilot = float(rng.uniform(8.0, 30.0))
    actual = pilot
    lb, ub = np.zeros(Tm), rng.uniform(20.0, 32.0, Tm)
    if kind == 0:      # no slot; the estimate of a session that left is forgotten
        ln, est = 0, 7.0
    elif kind == 1:    # a slot that has not arrived
        off, est = int(rng.integers(1, 4)), 9.0
    elif kind == 2:    # a window longer than the horizon
        ln, est = Tm + int(rng.integers(1, 4)), 11.0
    elif kind == 3:    # first sight
        fresh, est = 1, math.inf
    elif kind == 4:    # a fresh mark on an empty slot
        ln, fresh, est = 0, 1, math.inf
    elif kind == 5:    # ramp down: clearly less was drawn than offered
        actual = pilot - DOWN - float(rng.uniform(0.5, 6.0))
    elif kind == 6:    # ramp up: the bound was offered and drawn
        est = pilot
    elif kind == 7:    # hold: a little less drawn than offered, far from the bound
        actual = pilot - 0.5 * DOWN
    elif kind == 8:    # ON the down threshold to the bit: not a ramp down
        actual = float(rng.integers(16, 80)) / 4
        pilot = actual + DOWN
    elif kind == 9:    # ON the up threshold to the bit: not a ramp up
        pilot = actual = float(rng.integers(16, 80)) / 4
        est = actual + UP
    elif kind == 10:   # a bound above every ub
        est = 100.0
    elif kind == 11:   # a bound between the bounds of two periods
        ub[:] = np.where(np.arange(Tm) % 2 == 0, 32.0, 8.0)
        ln, est, pilot, actual = Tm, 16.0, 4.0, 4.0
    elif kind == 12:   # a bound below lb: reconciled to lb
        lb[:] = 8.0
        est, pilot, actual = 5.0, 2.0, 2.0
    elif kind == 13:   # nothing was offered
        pilot, actual, est = float(rng.choice([0.0, -1.0])), 0.0, 12.0
    elif kind == 14:   # a window that fills the horizon
        ln = Tm
    elif kind == 15:   # an estimate that is still +inf on a session seen before (a first step without a fresh mark)
        est = math.inf
    return off, ln, fresh, est, pilot, actual, lb, ub


def n_calls(N, B):
    return max(4, -(-120 // (B * N)))


@functools.lru_cache(maxsize=None)
def calls(N, B, Tm):
    """the calls of shape (N, B, Tm): a tuple of dicts cur (s_off, s_len (B, 1, N); lb, ub (B, N, Tm)), fresh, est, and the
    history pilots, actual, status -- each of the three may be None"""
    rng = np.random.default_rng(100000 * Tm + 1000 * N + B)
    S = n_calls(N, B)
    out = []
    for s in range(S):
        off, ln, fresh = (np.empty((B, N), np.int32) for _ in range(3))
        est, pilots, actual = np.empty((B, N)), np.empty((B, N)), np.empty((B, N))
        lb, ub = np.empty((B, N, Tm)), np.empty((B, N, Tm))
        status = np.ones(B, np.int32)
        for b in range(B):
            q = s * B + b
            if q % 7 == 3 or (B == 1 and s == 1):
                status[b] = (2, 3, 0, 4)[q % 4]          # MAX_ITER, PRIMAL_INFEASIBLE, UNSET, EMPTY_SET
            elif q % 3 == 2:
                status[b] = spec.SOLVED_INACCURATE
            for i in range(N):
                kind = (q * N + i) % N_SITUATIONS
                if q % 5 == 2 and kind in (2, 4):             # one problem in five holds nothing to flag: its flag is 0
                    kind = 7
                off[b, i], ln[b, i], fresh[b, i], est[b, i], pilots[b, i], actual[b, i], lb[b, i], ub[b, i] = _element(kind, rng, Tm)
        call = dict(cur=dict(s_off=off.reshape(B, 1, N), s_len=ln.reshape(B, 1, N), lb=lb, ub=ub), fresh=fresh, est=est, pilots=pilots,
                    actual=actual, status=status)
        if s % 8 == 3:
            call.update(pilots=None, actual=None, status=None)   # no history: the first step of a run
        elif s % 4 == 2:
            call.update(actual=None)                             # no plant
        out.append(call)
    return tuple(out)


def run_spec(c, **replace):
    c = dict(c, **replace)
    return spec.estimate(c["cur"], c["fresh"], c["pilots"], c["actual"], c["status"], UP, DOWN, INC, c["est"])


@functools.lru_cache(maxsize=None)
def answers(N, B, Tm):
    """tests/estimate_spec.py on every call of the shape, computed once"""
    return tuple(run_spec(c) for c in calls(N, B, Tm))


def branches(c, w, up=UP, down=DOWN):
    """{branch: a (B, N) or (B,) mask} of one call ``c`` and the specification's answer ``w``, read from the data"""
    B, N, Tm = c["cur"]["ub"].shape
    off, ln = c["cur"]["s_off"].reshape(B, N), c["cur"]["s_len"].reshape(B, N)
    lb, ub = c["cur"]["lb"], c["cur"]["ub"]
    fresh = c["fresh"] != 0
    present = (ln > 0) & (off == 0) & (ln <= Tm)
    history = c["pilots"] is not None
    served = (np.ones(B, bool) if c["status"] is None else np.isin(c["status"], (spec.SOLVED, spec.SOLVED_INACCURATE)))[:, None] & np.ones((B, N), bool)
    update = present & ~fresh & history
    m = {}
    m["absent slot"] = ln <= 0
    m["future slot"] = (ln > 0) & (off > 0)
    m["window longer than Tm"] = ln > Tm
    m["fresh and present"] = fresh & present
    m["fresh and absent"] = fresh & ~present
    m["no history"] = present & ~fresh & (not history)
    m["status rejected"] = update & ~served
    inaccurate = np.zeros(B, bool) if c["status"] is None else c["status"] == spec.SOLVED_INACCURATE
    m["status inaccurate"] = update & inaccurate[:, None]
    m["actual NULL"] = update & (c["actual"] is None)
    if history:
        pp = np.where(served & (c["pilots"] > 0), c["pilots"], 0.0)
        pr = pp if c["actual"] is None else np.where(served, c["actual"], 0.0)
        with np.errstate(invalid="ignore"):
            ramp_down = update & (pp - pr > down)
            ramp_up = update & ~ramp_down & (c["est"] - pr < up)
            m["pp - pr == down_threshold"] = update & (pp - pr == down)
            m["u - pr == up_threshold"] = update & ~ramp_down & (c["est"] - pr == up)
    else:
        ramp_down = ramp_up = np.zeros((B, N), bool)
        m["pp - pr == down_threshold"] = m["u - pr == up_threshold"] = ramp_down
    m["ramp down"], m["ramp up"], m["hold"] = ramp_down, ramp_up, update & ~ramp_down & ~ramp_up
    inside = present[:, :, None] & (np.arange(Tm)[None, None, :] < ln[:, :, None])
    u = w["est"][:, :, None]
    m["cap above every ub"] = present & ~(inside & (u < ub)).any(2)
    m["cap between per-period ub values"] = (inside & (u < ub)).any(2) & (inside & (u >= ub)).any(2)
    m["cap below lb"] = (inside & (u < lb) & (w["ub"] == lb) & (lb <= ub)).any(2)
    m["s_len == Tm"] = present & (ln == Tm)
    m["s_len < Tm"] = present & (ln < Tm)
    m["flag bad fresh"] = (w["flags"] & spec.BAD_FRESH) != 0
    m["flag bad slot"] = (w["flags"] & spec.BAD_SLOT) != 0
    m["no flag"] = w["flags"] == 0
    return m


IMPOSSIBLE_AT_TM_1 = ("cap between per-period ub values", "s_len < Tm")


def occurrences(N, B, Tm):
    """{branch: how often it occurs over the calls of the shape}"""
    count = {}
    for c, w in zip(calls(N, B, Tm), answers(N, B, Tm)):
        for k, mask in branches(c, w).items():
            count[k] = count.get(k, 0) + int(np.count_nonzero(mask))
    return count


def check_occurrences(N, B, Tm):
    count = occurrences(N, B, Tm)
    missing = [k for k, v in count.items() if v == 0 and not (Tm == 1 and k in IMPOSSIBLE_AT_TM_1)]
    assert not missing, (N, B, Tm, missing)
    return count


def handle_of(N):
    """a handle of a synthetic site of ``N`` EVSEs behind one row (the estimator entries read only N of it)"""
    from tests import plant_cases

    return plant_cases.handle_of(N)
