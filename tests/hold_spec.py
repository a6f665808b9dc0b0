"""The two rule lists of acnqp_select_device and acnqp_hold_device (include/acn_qp.h, "select and hold") in plain Python
loops, one problem at a time.  This is the yardstick: the kernels (adacharge_amd/csrc/acn_qp_hold.hpp) are held to it bit for
bit.  Nothing here computes: every element is a copy, a constant, or the outcome of two comparisons.

A closed loop that re-solves a scenario only on events (rollout.FleetTable.resolve_rows) takes the resolving scenarios
out of the resident state into a dense batch (select), solves that batch, and puts the answers back beside the held
schedules of everyone else (hold).  Which scenario resolves is decided before the run: neither rule list reads an answer
to decide anything."""
import numpy as np

SELECT_BAD_INDEX = 1
HOLD_BAD_ROW = 1
PER_EVSE_PERIOD = ("lb", "ub", "q")          # (B, N, Tm)
PER_SLOT = ("s_off", "s_len", "s_cap")       # (B, K, N)
SCALARS = ("horizon", "pdiag", "s_eq", "lf", "dc", "dfloor")   # (B,)
EMPTY = dict(horizon=1, peak=np.inf)         # what DeviceBatch.empty holds where it does not hold zero


def select(cur, idx, warm_x=None, warm_y=None):
    """Rules S1 and S2.  ``cur``: dict of the arrays of ``acnqp_problems`` -- horizon, lb, ub, q, pdiag, s_off, s_len, s_cap,
    s_eq and, where the site has the row, peak, lf, dc, dfloor -- of B problems; ``idx``: (m,) int32; ``warm_x`` (B, N, Tm) and
    ``warm_y`` (B, Mg, Tm) when wanted.  Returns a dict of the same arrays for the m problems of the dense batch, ``warm_x`` /
    ``warm_y`` when given and ``flags`` (m,) int32; nothing given is changed."""
    B, m = len(cur["horizon"]), len(idx)
    src = dict(cur)
    if warm_x is not None:
        src["warm_x"] = warm_x
    if warm_y is not None:
        src["warm_y"] = warm_y
    out = {k: np.empty((m,) + np.shape(a)[1:], np.asarray(a).dtype) for k, a in src.items()}
    flags = np.empty(m, np.int32)
    for j in range(m):
        b = int(idx[j])
        if 0 <= b < B:                                   # S1: a copy, bit for bit
            for k, a in src.items():
                out[k][j] = a[b]
            flags[j] = 0
        else:                                            # S2: the empty problem
            for k in src:
                out[k][j] = EMPTY.get(k, 0)
            flags[j] = SELECT_BAD_INDEX
    out["flags"] = flags
    return out


def clip(v, lb, ub):
    """rule H2 for one element: two comparisons, in this order; what is returned is one of the three arguments"""
    if v > ub:
        v = ub
    if v < lb:
        v = lb
    return v


def hold(pos, m, rx, rstatus, riters, held_x, prev_status, lb, ub, ry=None, held_y=None):
    """Rules H1 - H3.  ``pos``: (B,) int32; the dense results ``rx`` (m, N, Tm), ``rstatus``, ``riters`` (m,) and ``ry``
    (m, Mg, Tm) when wanted; the held schedule ``held_x`` (B, N, Tm) and ``held_y`` (B, Mg, Tm) when wanted; ``prev_status``
    (B,); the state's ``lb``, ``ub`` (B, N, Tm).  Returns a dict of x (B, N, Tm), status, iters (B,) int32, solved (B,) uint8,
    flags (B,) int32 and, when wanted, y (B, Mg, Tm); nothing given is changed."""
    B, N, Tm = np.shape(held_x)
    x = np.empty((B, N, Tm))
    y = None if held_y is None else np.empty(np.shape(held_y))
    status, iters, flags = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    solved = np.empty(B, np.uint8)
    for b in range(B):
        j = int(pos[b])
        if 0 <= j < m:                                   # H1
            x[b] = rx[j]
            if y is not None:
                y[b] = ry[j]
            status[b], iters[b], solved[b], flags[b] = rstatus[j], riters[j], 1, 0
        else:                                            # H2, and H3 for a row that is neither -1 nor a row
            for i in range(N):
                for t in range(Tm):
                    x[b, i, t] = clip(held_x[b, i, t], lb[b, i, t], ub[b, i, t])
            if y is not None:
                y[b] = held_y[b]
            status[b], iters[b], solved[b] = prev_status[b], 0, 0
            flags[b] = 0 if j == -1 else HOLD_BAD_ROW
    out = dict(x=x, status=status, iters=iters, solved=solved, flags=flags)
    if y is not None:
        out["y"] = y
    return out


def inverse(idx, B):
    """pos (B,) int32 of a strictly increasing ``idx``: pos[idx[j]] = j, -1 elsewhere"""
    pos = np.full(B, -1, np.int32)
    pos[np.asarray(idx, np.int64)] = np.arange(len(idx), dtype=np.int32)
    return pos
