"""Calls for the direct path for x (adacharge_amd/csrc/acn_qp_pipeline.hpp): the wave kernel stores
a problem's schedule straight into a PINNED result array; pageable result arrays keep the copies.  A plain module, like
wave_cases.py: tests/test_direct_x_gpu.py solves every call both ways in one process and compares the bits; run as a
script it solves the named calls with pinned result arrays under the environment it was started with
(ACNQP_NO_DIRECT_X=1: the copy path everywhere) and saves the results and what acnqp_debug_direct_x reported.

A call is (batches of ONE site and shape, options, warm starts or None).  Every call runs on the route `wave1`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEYS = ("x", "status", "iters", "pri_res", "dua_res", "obj")
CHILD_CALLS = ("n7_t5", "pieces")   # what the child process of the test solves


def _objective(w=1e-3):
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge

    return [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, w)]


def _feeder_batches(n, limit, horizon, sizes, seed, horizons=None):
    """batches of `sizes` problems on n EVSEs behind one feeder; horizons[k % len]: the horizon problem k is drawn for"""
    from adacharge_amd import sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch, make_site

    from tests.verdict_cases import feeder_site

    infra = feeder_site([n], [limit])
    iface = Interface({"infrastructure_info": infra, "period": 5})
    site = make_site(infra, "SOC")
    rng = np.random.default_rng(seed)
    hz = horizons or (horizon,)
    out, k = [], 0
    for b in sizes:
        snaps = []
        for _ in range(b):
            snaps.append(sites.random_sessions(infra, hz[k % len(hz)], rng, min_sessions=max(1, n // 2)))
            k += 1
        if horizons:   # (the batch's t_max is the largest horizon of its problems: one of full length in every batch)
            snaps[0] = sites.random_sessions(infra, horizon, rng, min_sessions=max(1, n // 2))
        out.append(build_batch(snaps, infra, iface, _objective(), "SOC", site=site))
        assert out[-1].Tm == horizon and out[-1].K == 1
    return out


def _caltech(horizon, sizes, seed, w=1e-3):
    from adacharge_amd import sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch, make_site

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    site = make_site(infra, "SOC")
    return [build_batch(sites.snapshot_batch(infra, horizon, b, seed=seed + 17 * g), infra, iface, _objective(w), "SOC", site=site)
            for g, b in enumerate(sizes)]


def build(name):
    """(batches, options, warm)"""
    from adacharge_amd.backend import default_options

    if name == "n1_t1":       # one EVSE, one period: one double per problem
        return _feeder_batches(1, 20.0, 1, (5, 4), 101), default_options(), None
    if name == "n7_t5":       # 35 doubles: one partial store, problems not 16-byte aligned
        return _feeder_batches(7, 90.0, 5, (9, 6), 102), default_options(), None
    if name == "n54_t12":     # the headline shape: 648 doubles, ten full stores and one of 8 lanes
        return _caltech(12, (40, 24), 103), default_options(), None
    if name == "n64_t12":     # every lane an EVSE: twelve full stores
        return _feeder_batches(64, 700.0, 12, (20, 13), 104), default_options(), None
    if name == "short_horizons":   # problems whose own horizon is shorter than the batch's t_max
        b = _feeder_batches(7, 90.0, 12, (11, 8), 105, horizons=(12, 5, 9, 3))
        assert any((x.T < x.Tm).any() for x in b)
        return b, default_options(), None
    if name == "pieces":      # with ACNQP_PLAN=3,4: chunks of 3, 4 and 6 over batches of 5, 1 and 7
        return _feeder_batches(7, 90.0, 5, (5, 1, 7), 106), default_options(), None
    if name == "verdicts":    # an empty-set problem and a certified-infeasible one among problems that solve
        from tests import verdict_cases as V

        rng = np.random.default_rng(107)
        fill = V.solved_filler("n8", "SOC", rng, 3)
        empty = V.empty_session(1, "first", "ub_eq", 1e-2, site="n8", cone="SOC")
        infeasible = V.feeder_equalities("n8", "SOC", 1e-2)
        assert (empty.expected, infeasible.expected) == (4, 3)
        return [fill[0], empty.batch, fill[1], infeasible.batch, fill[2]], default_options(), None
    if name == "hand_over":   # tests/polish_alongside_cases.py, `one_per_wave`: a fifth of the problems run past 300 iterations
        return _caltech(12, (128, 128), 9302, w=1e-12), default_options(polish_iters=300), None
    if name == "launch_order":   # 800 problems of an 8-EVSE x 4-period site in batches of 100: the launch order is active
        return _feeder_batches(8, 100.0, 4, (100,) * 8, 108), default_options(), None
    raise KeyError(name)


def results_of(results):
    return {k: np.concatenate([np.asarray(getattr(r, k)).reshape(r.x.shape[0], -1) for r in results]) for k in KEYS}


def solve(h, batches, options, pinned, warm=None):
    """One call of acnqp_solve_batches; pinned[g]: batch g's result arrays are pinned, their x pre-filled with NaN so that
    an element nobody wrote shows.  Returns (outputs, acnqp_debug_direct_x)."""
    run, results = h.prepare_many(batches, pinned_results=pinned, warm=warm)
    for r, p in zip(results, pinned):
        if p:
            r.x[...] = np.nan
    run(options)
    return results_of(results), h.direct_x()


if __name__ == "__main__":
    from adacharge_amd.backend import SiteHandle

    flat = {}
    for name in CHILD_CALLS:
        batches, options, warm = build(name)
        h = SiteHandle(batches[0].site, 0)
        out, direct = solve(h, batches, options, [True] * len(batches), warm)
        h.close()
        flat.update({f"{name}:{k}": v for k, v in out.items()})
        flat[f"{name}:direct"] = np.int64(direct)
    np.savez_compressed(sys.argv[1], **flat)
