"""tests/polish_long_cases.py on the CPU: every line of its table re-proved from the C twin (oracle/admm_port) and the
polish's specification (oracle/polish_ref.py with MAX_ROWS raised to the worst case of the shape, MAX_ROUNDS = 96
unchanged).  A condition on the INPUTS of tests/test_polish_long_gpu.py: a pool that misses it is changed, or its P -- never
the threshold."""
import numpy as np
import pytest

from tests import polish_long_cases as LC

CASES = list(LC.CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_pool_is_open_at_p_and_the_specification_does_what_the_case_says(case):
    name, P, expect, late, _ = LC.CASES[case]
    assert P % LC.CHECK_EVERY == 0 and late == (P >= 100)
    pool, c = LC.pool(name), LC.cpu_case(case)
    feasible = [b for b in c["index"] if c["final"]["status"][b] != 3]
    accepted = [b for b in feasible if c["spec"][b][1]["ok"]]
    why = {b: c["spec"][b][1]["why"] for b in c["index"] if not c["spec"][b][1]["ok"]}
    rounds = max((c["spec"][b][1]["rounds"] for b in accepted), default=0)
    rows = max((c["spec"][b][1]["rows"] for b in c["index"]), default=0)
    print(f"[polish-long] {case}: Tm {pool.Tm}, K {pool.K}, Mg {pool.site.Mg}; open at P {len(c['index'])} of {pool.B}, feasible "
          f"{len(feasible)}, accepted {len(accepted)}, rounds <= {rounds}, give-ups {why}, rows <= {rows} of {LC.worst_rows(pool.site, pool.Tm)}, "
          f"block doubles <= {max((c['spec'][b][1].get('blocks', 0) for b in c['index']), default=0)}")
    assert len(c["index"]) >= 2, "the problems must be open at P"
    assert "rows" not in why.values() and rows <= LC.worst_rows(pool.site, pool.Tm)
    if expect == "accept":
        assert feasible and 4 * len(accepted) >= 3 * len(feasible), (len(accepted), len(feasible), why)
    else:
        assert accepted and "rounds" in why.values(), why
    for b in accepted:   # accepted answers are the twin's converged ones
        T = int(pool.T[b])
        if c["final"]["status"][b] == 1:
            assert np.abs(c["spec"][b][0] - c["final"]["x"][b][:, :T]).max() <= 1e-4, (case, b)


def test_the_shapes_cover_what_can_go_wrong_at_a_long_horizon():
    """33; 48 | 49 (the family boundary); 65 (past a 64-bit word of periods); >= 257 (past 8 bits); a short last strip; K = 4;
    lb == ub; scalar and vector peak; both cones"""
    horizons, shapes, kinds = set(), set(), set()
    for case in CASES:
        pool = LC.pool(LC.CASES[case][0])
        horizons |= {int(t) for t in pool.T}
        shapes |= set(LC.shapes(case))
        kinds.add("soc" if int(pool.site.cone) == 1 else "linear")
        if pool.K == 4 and pool.s_len[:, 3].any():
            kinds.add("four_sessions")
        live = np.arange(pool.Tm)[None, None, :] < np.asarray(pool.T)[:, None, None]
        if ((pool.lb == pool.ub) & (pool.lb > 0) & live).any():
            kinds.add("pinned")
        if pool.peak is not None:
            for b in range(pool.B):
                pk = pool.peak[b][: int(pool.T[b])]
                if np.isfinite(pk).all():
                    kinds.add("scalar_peak" if np.ptp(pk) == 0 else "vector_peak")
    ts = {t for t, _ in shapes}
    assert {33, 65} <= horizons and max(horizons) >= 257, sorted(horizons)
    assert {48, 49, 288} <= ts and any(t % 4 for t in ts) and any(k == 4 for _, k in shapes), sorted(shapes)
    assert {"soc", "linear", "four_sessions", "pinned", "scalar_peak", "vector_peak"} <= kinds, sorted(kinds)
