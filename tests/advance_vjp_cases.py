"""Inputs for tests of the adjoint of time passes (tests/advance_vjp_spec.py, acnqp_advance_vjp_device): the hand cases, one
rule each with the expected values written out, and random states that meet every branch of the replay."""
import numpy as np

NO_ROW = 2


def hand_case():
    """Three copies of one state (N = 4, K = 1, t_max = 4) after period 1: b0 solved, b1 not solved (status 2), b2 solved
    but its next state had no objective row (flags_next NO_ROW).  EVSE 0: a slot that starts later (off 1); EVSE 1: a
    served slot that is kept; EVSE 2: a served slot whose cap the delivery exceeds (clamped at 0 and dropped); EVSE 3:
    idle, its schedule entry above max_pilot, and an arrival.  Returns (args of advance_vjp_spec.advance_vjp, expected)."""
    B, N, K, Tm, P = 3, 4, 1, 4, 8
    one = lambda v, dt=float: np.repeat(np.array([[v]], dtype=dt), B, axis=0)   # (B, K, N)
    cur = dict(s_off=one([1, 0, 0, 0], np.int32), s_len=one([2, 3, 2, 0], np.int32), s_cap=one([5.0, 10.0, 3.0, 0.0]))
    applied = np.repeat(np.array([[0.0, 4.0, 5.0, 0.0]]), B, axis=0)
    status = np.array([1, 2, 1], np.int32)
    x = np.zeros((B, N, Tm))
    x[:, :, 0] = [0.0, 4.0, 5.0, 40.0]
    max_pilot = np.full(N, 32.0)
    gdir = np.repeat(np.array([[10.0, 20.0, 30.0, 40.0]]), B, axis=0)
    # records: b0: EVSE 3 (free: admitted), EVSE 1 (its slot is live: refused); b1: EVSE 3 with a length beyond t_max (refused)
    plan = dict(step=1, t_max=Tm, done_tol=1e-6, a_seg=np.array([0, 2, 3, 3], np.int32), a_evse=np.array([3, 1, 3], np.int32),
                a_slot=np.zeros(3, np.int32), a_len=np.array([2, 2, 5], np.int32), a_cap=np.array([7.0, 7.0, 7.0]),
                a_rate_seg=np.array([0, 2, 4, 9], np.int32), a_min=np.zeros(9), a_max=np.full(9, 32.0))
    cost = dict(coef=2.0, weight=np.array([1.0, 2.0, 3.0, 4.0]), series_len=P)
    gq = np.zeros((B, N, Tm))
    for i in range(N):
        for t in range(Tm):
            gq[:, i, t] = 0.5 * (i + 1) * (t + 1)
    nxt = dict(gq=gq, gcap_vjp=one([1.0, 2.0, 3.0, 4.0]), gcap_carry=one([0.5, 0.25, 0.125, 8.0]),
               horizon=np.array([2, 3, 2], np.int32), flags=np.array([0, 0, NO_ROW], np.int32))
    garr0, gprice0 = np.full(3, -1.0), np.ones((B, P))
    # A1: G = [1.5, 2.25, 3.125, 12]
    expect = dict(
        # A4: off > 0 kept; served and kept; clamped and dropped; empty.  b1 delivered nothing: EVSE 2 keeps cap 3 and is kept
        gcap_carry=np.array([[[1.5, 2.25, 0.0, 0.0]], [[1.5, 2.25, 3.125, 0.0]], [[1.5, 2.25, 0.0, 0.0]]]),
        # A5: gdir, gdir - G for the kept served slot, gdir, gdir; A6: EVSE 3 sits above max_pilot; b1 is not served
        gx0=np.array([[10.0, 17.75, 30.0, 0.0], [0.0, 0.0, 0.0, 0.0], [10.0, 17.75, 30.0, 0.0]]),
        # A7: admitted into (0, 3): G = 12; refused: 0
        garr=np.array([12.0, 0.0, 0.0]),
        # A2: acc_t = 0.5 (t + 1) (1 + 4 + 9 + 16) = 15 (t + 1), times coef 2, onto the ones, from period step + 1 = 2
        gprice=np.array([[1, 1, 31, 61, 1, 1, 1, 1], [1, 1, 31, 61, 91, 1, 1, 1], [1] * 8], dtype=float),
    )
    return dict(cur=cur, applied=applied, status=status, x=x, max_pilot=max_pilot, plan=plan, cost=cost, gdir=gdir, nxt=nxt,
                garr=garr0, gprice=gprice0), expect


def random_case(N, K, Tm, B, seed, clock=True, step=2, with_next=True):
    """A batch of random states, arrivals and adjoints: live, empty, later and out-of-range slots; deliveries below, at and
    above the cap; records that are admitted and records refused for every reason; a NO_ROW flag; unsolved problems;
    schedule entries below 0 and above max_pilot.  ``step`` -1: the empty state and its arrivals only.  Returns the
    arguments of ``advance_vjp_spec.advance_vjp`` as a dict."""
    rng = np.random.default_rng(seed)
    P = max(step, 0) + 1 + Tm + 3
    first = step < 0
    off = rng.integers(0, Tm, (B, K, N)).astype(np.int32)
    ln = np.minimum(rng.integers(0, Tm + 1, (B, K, N)), Tm - off).astype(np.int32)
    off[rng.random((B, K, N)) < 0.5] = 0
    ln = np.minimum(ln, Tm - off).astype(np.int32)
    ln[rng.random((B, K, N)) < 0.3] = 0
    bad = rng.random((B, K, N)) < 0.05
    off[bad], ln[bad] = Tm - 1, 3   # not a window of this horizon (for Tm >= 3)
    cap = rng.uniform(0.0, 40.0, (B, K, N))
    applied = rng.uniform(0.0, 32.0, (B, N))
    exact = rng.random((B, N)) < 0.2
    applied[exact] = cap[:, 0, :][exact]   # delivers the cap of slot 0 exactly: cap' = 0 <= done_tol
    if first:
        off[:], ln[:], cap[:] = 0, 0, 0.0
    status = rng.choice([1, 1, 1, 5, 2, 3], B).astype(np.int32)
    x = rng.uniform(-2.0, 36.0, (B, N, Tm))
    max_pilot = rng.choice([16.0, 32.0], N)
    # arrivals: about one record per two EVSEs and problem, some with a bad EVSE, slot, length or rate segment
    n_rec = rng.integers(0, N // 2 + 2, B)
    seg = np.zeros(B + 1, np.int32)
    np.cumsum(n_rec, out=seg[1:])
    A = int(seg[-1])
    a_evse = rng.integers(0, N, A).astype(np.int32)
    a_slot = rng.integers(0, K, A).astype(np.int32)
    a_len = rng.integers(1, Tm + 1, A).astype(np.int32)
    for arr, vals in ((a_evse, (-1, N)), (a_slot, (-1, K)), (a_len, (0, Tm + 1))):
        hit = rng.random(A) < 0.06
        arr[hit] = rng.choice(vals, int(hit.sum()))
    rate_seg = np.zeros(A + 1, np.int32)
    np.cumsum(np.maximum(a_len, 0), out=rate_seg[1:])
    R = int(rate_seg[-1])
    if A:
        rate_seg[-2] = max(R - 1, 0) if rng.random() < 0.5 else rate_seg[-2]   # (its entries may leave the rate arrays)
    plan = dict(step=step, t_max=Tm, done_tol=1e-6, a_seg=seg, a_evse=a_evse, a_slot=a_slot, a_len=a_len, a_cap=rng.uniform(1.0, 40.0, A),
                a_rate_seg=rate_seg, a_min=np.zeros(R), a_max=np.full(R, 32.0))
    cost = dict(coef=float(rng.normal()), weight=rng.uniform(0.01, 0.03, N), series_len=P) if clock else None
    nxt = None
    if with_next:
        flags = np.zeros(B, np.int32)
        flags[rng.random(B) < 0.15] = NO_ROW
        flags[rng.random(B) < 0.15] |= 1
        nxt = dict(gq=rng.standard_normal((B, N, Tm)), gcap_vjp=rng.standard_normal((B, K, N)), gcap_carry=rng.standard_normal((B, K, N)),
                   horizon=rng.integers(1, Tm + 1, B).astype(np.int32), flags=flags)
    return dict(cur=dict(s_off=off, s_len=ln, s_cap=cap), applied=None if first else applied, status=None if first else status,
                x=None if first else x, max_pilot=None if first else max_pilot, plan=plan, cost=cost,
                gdir=None if first else rng.standard_normal((B, N)), nxt=nxt, garr=rng.standard_normal(A),
                gprice=rng.standard_normal((B, P)) if clock else None)


def run_spec(case):
    from tests import advance_vjp_spec as AV

    return AV.advance_vjp(case["cur"], case["applied"], case["status"], case["x"], case["max_pilot"], case["plan"], case["cost"],
                          case["gdir"], case["nxt"], case["garr"], case["gprice"])
