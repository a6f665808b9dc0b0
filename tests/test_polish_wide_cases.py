"""tests/polish_wide_cases.py on the CPU: every line of its table re-proved from the C twin (oracle/admm_port) stopped by the
case's start options and the polish's specification (oracle/polish_ref.py with MAX_ROWS raised to the worst case of the
shape, MAX_ROUNDS = 96 unchanged).  A condition on the INPUTS of tests/test_polish_wide_gpu.py: a pool that misses it is
changed, or its start -- never the threshold."""
import collections

import numpy as np
import pytest

from tests import polish_wide_cases as WC

CASES = list(WC.CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_pool_is_open_at_the_start_and_the_specification_does_what_the_case_says(case):
    name, start, pads, late, (n_open, n_acc, max_rounds, give_ups) = WC.CASES[case]
    assert start["max_iter"] % WC.CHECK_EVERY == 0 and late == ("eps_abs" in start)
    pool, c = WC.pool(name), WC.cpu_case(case)
    site = pool.site
    assert 64 < site.N <= 1024 and pool.Tm <= 48 and pool.K <= 4 and site.Mg <= 48 and not site.has_flat and not site.has_max
    assert all(t <= 48 and k <= 4 and 8 * ((site.N * k + 7) // 8) <= 1024 for t, k in WC.shapes(case)), WC.shapes(case)
    accepted = [b for b in c["index"] if c["spec"][b][1]["ok"]]
    why = collections.Counter(c["spec"][b][1]["why"] for b in c["index"] if not c["spec"][b][1]["ok"])
    rounds = max((c["spec"][b][1]["rounds"] for b in accepted), default=0)
    rows = max((c["spec"][b][1]["rows"] for b in c["index"]), default=0)
    cols = max((c["spec"][b][1].get("sessions", 0) for b in c["index"]), default=0)
    print(f"[polish-wide] {case}: N {site.N}, Tm {pool.Tm}, K {pool.K}, Mg {site.Mg}; open {len(c['index'])} of {pool.B}, accepted "
          f"{len(accepted)}, rounds <= {rounds}, give-ups {dict(why)}, rows <= {rows} of {WC.LC.worst_rows(site, pool.Tm)}, session columns <= {cols}")
    assert len(c["index"]) == n_open and len(accepted) == n_acc, (len(c["index"]), len(accepted), dict(why))
    assert rounds <= max_rounds and dict(why) == give_ups, (rounds, dict(why))
    assert rows <= WC.LC.worst_rows(site, pool.Tm) and cols <= 8 * ((site.N * pool.K + 7) // 8)
    if late:   # the ADMM's last iterate: a handful of rounds
        assert rounds <= 3
    for b in accepted:   # accepted answers are the twin's converged ones (1e-3 A: what the reference's tests accept)
        T = int(pool.T[b])
        if c["final"]["status"][b] == 1:
            assert np.abs(c["spec"][b][0] - c["final"]["x"][b][:, :T]).max() <= 1e-3, (case, b)
    if give_ups.get("verify"):   # the instance the final check rejects is one the twin calls infeasible
        bad = [b for b in c["index"] if c["spec"][b][1]["why"] == "verify"]
        assert all(c["final"]["status"][b] == 3 for b in bad), [int(c["final"]["status"][b]) for b in bad]


def test_the_shapes_cover_what_can_go_wrong_on_a_wide_site():
    """65; a short second tile; a third tile; 1,024 (the last tile full); K = 4; lb == ub; both cones; scalar, vector and no
    peak; horizon 48 and horizons that are no multiple of four; more session columns than the 256 threads of a workgroup"""
    sizes, ts, kinds = set(), set(), set()
    for case in CASES:
        pool = WC.pool(WC.CASES[case][0])
        sizes.add(int(pool.site.N))
        ts |= {t for t, _ in WC.shapes(case)}
        kinds.add("soc" if int(pool.site.cone) == 1 else "linear")
        if any(k == 4 for _, k in WC.shapes(case)) and pool.K == 4 and pool.s_len[:, 3].any():
            kinds.add("four_sessions")
        live = np.arange(pool.Tm)[None, None, :] < np.asarray(pool.T)[:, None, None]
        if ((pool.lb == pool.ub) & (pool.lb > 0) & live).any():
            kinds.add("pinned")
        if pool.peak is not None:
            for b in range(pool.B):
                pk = pool.peak[b][: int(pool.T[b])]
                kinds.add(("scalar_peak" if np.ptp(pk) == 0 else "vector_peak") if np.isfinite(pk).all() else "no_peak")
        if int((pool.s_len > 0).sum(axis=(1, 2)).max()) > 256:
            kinds.add("columns_beyond_256")
    assert {65, 1024} <= sizes and any(65 < n < 128 for n in sizes) and any(128 < n <= 192 for n in sizes), sorted(sizes)
    assert 48 in ts and any(t % 4 for t in ts) and 17 in ts and 33 in ts, sorted(ts)
    assert {"soc", "linear", "four_sessions", "pinned", "scalar_peak", "vector_peak", "columns_beyond_256"} <= kinds, sorted(kinds)
