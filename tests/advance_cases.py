"""Inputs shared by tests/test_advance_spec.py (CPU) and tests/test_advance_gpu.py: one batch of B = 7 problems per shape
that holds every unit case of the advance rules, built by hand (no solve: states, x and y are random).

  problem 0  a random state with valid arrivals (one on a free EVSE, one behind a window that ends in this step)
  problem 1  retirement: by length (len 1), by cap (applied == cap; cap - applied below done_tol), and a survivor
  problem 2  a future session (off > 0; with K = 2 behind a present one on the same EVSE) and an arrival in front of it
  problem 3  a random state, SOLVED_INACCURATE (the problem the tests also advance alone)
  problem 4  idle: no session at all (horizon' = 1, all bounds zero)
  problem 5  refused arrivals, one per reason, a slot outside [0, Tm), and -- for Tm >= 3 -- a horizon without a row
  problem 6  status MAX_ITER: time passes, nothing is delivered, dfloor stays
"""
import numpy as np

B = 7
SHAPES = ((54, 12, 1), (54, 24, 2), (70, 20, 1), (5, 1, 1))   # (N, Tm, K)
DONE_TOL = 1e-6


def _window(c, b, k, i, off, ln, cap, lo=0.0, hi=32.0):
    c["s_off"][b, k, i], c["s_len"][b, k, i], c["s_cap"][b, k, i] = off, ln, cap
    c["lb"][b, i, off:off + ln] = lo
    c["ub"][b, i, off:off + ln] = hi


def _random_state(c, b, rng, N, Tm, K, top):
    """windows that end at or before ``top`` (so that the problem's next horizon stays below top)"""
    for i in range(N):
        if top < 1 or rng.random() < 0.3:
            continue
        ln = int(rng.integers(1, top + 1))
        off = 0 if rng.random() < 0.7 else int(rng.integers(0, top - ln + 1))
        _window(c, b, 0, i, off, ln, float(rng.uniform(1.0, 32.0 * ln)), float(rng.choice([0.0, 1.0, 6.0])), float(rng.uniform(8.0, 32.0)))
        if K > 1 and off + ln < top and rng.random() < 0.5:
            ln2 = int(rng.integers(1, top - off - ln + 1))
            off2 = int(rng.integers(off + ln, top - ln2 + 1))
            _window(c, b, K - 1, i, off2, ln2, float(rng.uniform(1.0, 32.0 * ln2)), 0.0, float(rng.uniform(8.0, 32.0)))


def make(N, Tm, K, seed=0, Mg=3):
    """(cur, applied, status, x, y, plan): dicts / arrays in the layout tests/advance_spec.py takes."""
    rng = np.random.default_rng(1000 * seed + 100 * N + 10 * Tm + K)
    c = dict(lb=np.zeros((B, N, Tm)), ub=np.zeros((B, N, Tm)), s_off=np.zeros((B, K, N), np.int32),
             s_len=np.zeros((B, K, N), np.int32), s_cap=np.zeros((B, K, N)), dfloor=np.array([0.0, 2.0, 1e3, 0.5, 3.0, 0.0, 1.0]))
    top = Tm if Tm < 3 else Tm - 1   # (Tm >= 3) every window but one of problem 5 ends by Tm - 1: next horizon <= Tm - 2
    for b in (0, 3, 6):
        _random_state(c, b, rng, N, Tm, K, top)
    arr = []   # (problem, evse, slot, len, cap, min, max)

    def arrive(b, i, k, ln, lo=None, hi=None, cap=None):
        n = max(ln, 0)
        arr.append((b, i, k, ln, float(rng.uniform(5.0, 200.0)) if cap is None else cap,
                    rng.choice([0.0, 2.0], size=n) if lo is None else np.full(n, lo), rng.uniform(1.0, 32.0, size=n) if hi is None else np.full(n, hi)))

    alen = max(1, min(top - 1, 5))
    # 0: arrivals on free EVSEs, and one behind a window that ends now
    c["s_len"][0, :, :2] = 0
    c["lb"][0, :2], c["ub"][0, :2] = 0.0, 0.0
    _window(c, 0, 0, 1, 0, 1, 50.0)
    arrive(0, 0, 0, alen)
    arrive(0, 1, K - 1, alen, lo=6.0, hi=4.0)        # max < min: aco.py:75
    # 1: retirement
    _window(c, 1, 0, 0, 0, 1, 100.0)                   # by length
    _window(c, 1, 0, 1, 0, top, 20.0, 0.0, 32.0)       # by cap: applied == cap
    _window(c, 1, 0, 2, 0, top, 20.0, 0.0, 32.0)       # by cap: cap - applied = 5e-7 <= done_tol
    _window(c, 1, 0, 3, 0, top, 20.0, 1.0, 32.0)       # survives (when top > 1)
    _window(c, 1, 0, 4, 0, top, 10.0, 0.0, 32.0)       # applied above cap: clamped at 0, retired
    # 2: future sessions
    if Tm >= 2:
        _window(c, 2, K - 1, 0, 1, top - 1, 64.0, 0.0, 16.0)          # arrives next period
        if top >= 3:
            _window(c, 2, K - 1, 1, 2, top - 2, 64.0, 2.0, 16.0)
            if K > 1:
                _window(c, 2, 0, 1, 0, 2, 30.0, 0.0, 32.0)            # a present session in front of it
                arrive(2, 2, 0, 1)
                _window(c, 2, K - 1, 2, 3 if top > 3 else 2, 1 if top > 3 else top - 2, 9.0)
    # 5: refusals
    _window(c, 5, 0, 0, 0, top, 500.0)                 # live slot, and its window covers [0, len)
    arrive(5, 0, 0, 1)                                 # slot live
    if K > 1:
        arrive(5, 0, 1, 1)                             # free slot, but [0, 1) meets the live window
    arrive(5, N, 0, 1)                                 # EVSE out of range
    arrive(5, -1, 0, 1)
    arrive(5, 1, K, 1)                                 # slot out of range
    arrive(5, 1, 0, 0)                                 # length < 1
    arrive(5, 1, 0, Tm + 1)                            # length > Tm
    arrive(5, 1, 0, 1)                                 # admitted ...
    arrive(5, 1, 0, 1)                                 # ... so its twin is refused
    c["s_off"][5, 0, 2], c["s_len"][5, 0, 2], c["s_cap"][5, 0, 2] = Tm - 1, 2, 7.0   # a slot that leaves [0, Tm)
    c["s_off"][5, 0, 3], c["s_len"][5, 0, 3], c["s_cap"][5, 0, 3] = -1, 1, 7.0
    no_row = None
    if Tm >= 3:
        _window(c, 5, 0, 4, 0, Tm, 900.0)              # the only window that ends at Tm: horizon' = Tm - 1 has no row
        no_row = Tm - 1
    # applied pilots: what a feasible policy could have sent, and the retirement amounts of problem 1
    first = np.where(c["s_off"][:, 0, :] == 0, np.minimum(c["ub"][:, :, 0], c["s_cap"][:, 0, :]), 0.0) * (c["s_len"][:, 0, :] > 0)
    applied = first * rng.uniform(0.0, 1.0, size=(B, N))
    applied[1, :5] = [30.0, 20.0, 20.0 - 5e-7, 3.0, 12.0]
    status = np.array([1, 1, 1, 5, 1, 1, 2], np.int32)
    x, y = rng.uniform(0.0, 32.0, size=(B, N, Tm)), rng.normal(size=(B, Mg, Tm))
    # the plan
    H = Tm
    q_table = rng.normal(size=(H, N, Tm))
    h_scal = rng.uniform(0.0, 2.0, size=(H, 3))
    h_row = np.r_[-1, rng.permutation(H)].astype(np.int32)
    if no_row is not None:
        h_row[no_row] = -1
    order = sorted(range(len(arr)), key=lambda k: arr[k][0])
    arr = [arr[k] for k in order]
    seg = np.searchsorted([a[0] for a in arr], np.arange(B + 1)).astype(np.int32)
    lens = np.array([max(a[3], 0) for a in arr], np.int32)
    rate_seg = np.zeros(len(arr) + 1, np.int32)
    np.cumsum(lens, out=rate_seg[1:])
    step = 3
    plan = dict(q_table=q_table, h_scal=h_scal, h_row=h_row, done_tol=DONE_TOL, kw_per_amp=0.208, step=step,
                peak_series=rng.uniform(100.0, 500.0, size=(B, step + 1 + Tm + 2)), a_seg=seg,
                a_evse=np.array([a[1] for a in arr], np.int32), a_slot=np.array([a[2] for a in arr], np.int32),
                a_len=np.array([a[3] for a in arr], np.int32), a_cap=np.array([a[4] for a in arr]), a_rate_seg=rate_seg,
                a_min=np.concatenate([a[5] for a in arr]), a_max=np.concatenate([a[6] for a in arr]))
    return c, applied, status, x, y, plan, no_row


def subset(c, applied, status, x, y, plan, b):
    """problem ``b`` as a batch of its own (its arrival segment keeps absolute record indices)"""
    one = {k: v[b:b + 1].copy() for k, v in c.items()}
    p = dict(plan)
    p["a_seg"] = plan["a_seg"][b:b + 2].copy()
    p["peak_series"] = plan["peak_series"][b:b + 1].copy()
    return one, applied[b:b + 1].copy(), status[b:b + 1].copy(), x[b:b + 1].copy(), y[b:b + 1].copy(), p
