"""Calls for the direct path for lb / ub / q (adacharge_amd/csrc/acn_qp_pipeline.hpp): the wave kernel
loads the inputs of a call's LEADING chunk straight from PINNED host arrays; pageable arrays, later chunks and
ACNQP_NO_DIRECT_IN=1 keep the copies, and so does a call of ONE chunk (the path is gated off there: it measured a loss on a
call of 256 problems), so every case but `one_chunk` cuts its call in two with ACNQP_PLAN.  A plain module, like direct_x_cases.py: tests/test_direct_in_gpu.py solves a case
in its own process with the path on; run as a script (the test starts it once, with ACNQP_NO_DIRECT_IN=1) it solves EVERY
case the same way and saves the results and what acnqp_debug_direct_in reported.

A case is a list of calls on ONE handle, the last of which is compared; a call is (batches of one site and shape, options,
pin[g], warm).  pin[g]: "all" = lb, ub and q of batch g in pinned memory, "none" = pageable, "not_q" = q alone pageable."""
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import direct_x_cases as DC  # noqa: E402

KEYS = DC.KEYS
CASES = ("n64_t12", "n54_t12", "n5_t7", "n64_t1", "t12_after_t7", "hand_over", "hand_over_early", "retry", "verdicts", "mixed", "q_pageable",
         "two_chunks", "warm", "launch_order", "one_chunk")
# ACNQP_PLAN of the case (read at every call): the problems of the leading chunk; the rest of the call is the second chunk
PLAN = {"n64_t12": "9", "n54_t12": "9", "n5_t7": "9", "n64_t1": "9", "t12_after_t7": "5", "hand_over": "128", "hand_over_early": "64", "retry": "32",
        "verdicts": "4", "mixed": "14", "q_pageable": "8", "two_chunks": "128", "warm": "9", "launch_order": "780"}


def build(name):
    """([(batches, options, pin, warm), ...], problems the LAST call means to load directly); warm: None, or "self" = from the
    cold answers (x, y) of the same batches on the same handle"""
    from adacharge_amd.backend import default_options

    d = default_options()
    if name == "n64_t12":      # N Tm = 768, a multiple of 64: every lane live in every step; 9 problems: three workgroups, the last one of one wave
        return [(DC._feeder_batches(64, 700.0, 12, (9, 9), 204), d, ["all"] * 2, None)], 9
    if name == "n54_t12":      # the headline shape: 648 doubles, ten full steps and one of 8 lanes
        return [(DC._caltech(12, (9, 9), 203), d, ["all"] * 2, None)], 9
    if name == "n5_t7":        # 35 doubles: one partial step, problems not 16-byte aligned
        return [(DC._feeder_batches(5, 60.0, 7, (9, 9), 202), d, ["all"] * 2, None)], 9
    if name == "n64_t1":       # one period: 64 EVSE rows per step
        return [(DC._feeder_batches(64, 700.0, 1, (9, 9), 201), d, ["all"] * 2, None)], 9
    if name == "t12_after_t7":   # horizon 12 behind horizon 7 on one handle: nothing of the earlier call may show
        return [(DC._feeder_batches(5, 60.0, 7, (9,), 205), d, ["all"], None), (DC._feeder_batches(5, 60.0, 12, (9,), 206), d, ["all"], None)], 5
    if name == "hand_over":    # direct_x_cases `hand_over`: a quarter of the problems go to the polish, which reads the device copy
        return [(DC._caltech(12, (128, 128), 9302, w=1e-12), default_options(polish_iters=300), ["all"] * 2, None)], 128
    if name == "hand_over_early":   # ... after 100 iterations: more of them, further from their answers (what the polish gives up on is
        # passed on to the resume launch, which reads the device copy too; the project's stalled fixtures run on wave3)
        return [(DC._caltech(12, (128,), 9302, w=1e-12), default_options(polish_iters=100), ["all"], None)], 64
    if name == "retry":        # the same problems without a polish and with a pass 0 of 200 iterations: a retry pass reads the device copy
        return [(DC._caltech(12, (64,), 9302, w=1e-12), default_options(polish_iters=0, max_iter=200, stall_iters=100, retry_passes=1, retry_max_iter=400),
                 ["all"], None)], 32
    if name == "verdicts":     # an empty-set problem (status 4) and a certified-infeasible one among problems that solve
        batches, o, _ = DC.build("verdicts")
        return [(batches, o, ["all"] * len(batches), None)], 4   # (the first four of the five)
    if name == "mixed":        # a pinned and a pageable batch and 3 of the 7 problems of a pinned one behind it in the leading chunk
        return [(DC._feeder_batches(7, 90.0, 5, (5, 6, 7), 207), d, ["all", "none", "all"], None)], 8
    if name == "q_pageable":   # q alone pageable: the batch keeps all three copies; 3 of the 6 problems of the pinned one behind it
        return [(DC._feeder_batches(7, 90.0, 5, (5, 6), 208), d, ["not_q", "all"], None)], 3
    if name == "two_chunks":   # 300 problems of 8 EVSEs x 4 periods in chunks of 128 and 172: the leading chunk alone loads directly
        return [(DC._feeder_batches(8, 100.0, 4, (100,) * 3, 209), d, ["all"] * 3, None)], 128
    if name == "warm":         # warm start with multipliers
        b = DC._caltech(12, (9, 9), 210)
        return [(b, d, ["all"] * 2, None), (b, d, ["all"] * 2, "self")], 9
    if name == "launch_order":   # 780 of 800 problems in the leading chunk: the launch order is active, and by session count where the chunk loads directly
        batches, o, _ = DC.build("launch_order")
        return [(batches, o, ["all"] * len(batches), None)], 780
    if name == "one_chunk":    # a call of one chunk keeps its copies
        return [(DC._caltech(12, (9, 9), 211), d, ["all"] * 2, None)], 0
    raise KeyError(name)


def _pinned(a):
    from adacharge_amd.backend import pinned_empty

    p = pinned_empty(a.shape, a.dtype)
    p[...] = a
    return p


def pin(batch, how):
    if how == "none":
        return batch
    return dataclasses.replace(batch, lb=_pinned(batch.lb), ub=_pinned(batch.ub), q=_pinned(batch.q) if how == "all" else batch.q)


def solve(name):
    """The case's calls on one handle, every one with pinned result arrays; returns (outputs of the last call, its
    acnqp_debug_direct_in, the polish counters the last call added)."""
    from adacharge_amd.backend import SiteHandle

    calls, _ = build(name)
    if name in PLAN:
        os.environ["ACNQP_PLAN"] = PLAN[name]
    try:
        h = SiteHandle(calls[0][0][0].site, 0)
        results = None
        for batches, options, how, warm in calls:
            assert h.route(batches[0].Tm, batches[0].K, sum(b.B for b in batches))[0] == "wave1"
            batches = [pin(b, w) for b, w in zip(batches, how)]
            if warm == "self":
                cold = h.solve_many(batches, options, want_y=[True] * len(batches))
                warm = [(r.x.copy(), r.y.copy()) for r in cold]
            before = h.polish_stats()
            run, results = h.prepare_many(batches, pinned_results=True, warm=warm)
            run(options)
            after = h.polish_stats()
        out = DC.results_of(results), h.direct_in(), {k: after[k] - before[k] for k in ("attempted", "solved")}
        h.close()
        return out
    finally:
        os.environ.pop("ACNQP_PLAN", None)


if __name__ == "__main__":
    flat = {}
    for name in CASES:
        out, direct, _ = solve(name)
        flat.update({f"{name}:{k}": v for k, v in out.items()})
        flat[f"{name}:direct"] = np.int64(direct)
    np.savez_compressed(sys.argv[1], **flat)
