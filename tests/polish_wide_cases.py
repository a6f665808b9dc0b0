"""The wide-site polish kernel's pools (adacharge_amd/csrc/acn_qp_polish_wide.hpp: 64 < N <= 1,024, horizons <= 48, behind
the large-site kernel's launch), stated once: tests/test_polish_wide_cases.py proves on the CPU that they are fit for the job
and tests/test_polish_wide_gpu.py holds the kernel to oracle/polish_ref.py on them, problem by problem.  The pools are
tests.polish_cases.site_pool's, a site is (n, pods, frac) of sites.balanced_three_phase; the specification runs in
tests.polish_long_cases' workers, with its MAX_ROWS raised to the worst case of the shape (Mg t_max rows: the wide kernel's
tables hold it, nothing is ever given up for `rows`).  MAX_ROUNDS = 96 stays.

The wide polish starts BEHIND the solver launch: a case's start is the set of options under which the ADMM stops short --
``max_iter`` alone (the problems still open end MAX_ITER), or ``max_iter`` 800 with tolerances nothing meets (the `late`
cases: a wide site's working set changes by one constraint per round, and only a late iterate is within the 96 rounds).

CASES: case -> (pool, start options, pads, late, expect).  expect = (open, accepted, rounds at most among the accepted,
give-ups by reason) as measured on the CPU from the twin's iterate (tests/test_polish_wide_cases.py holds every line).
pads: (t_max, K) beyond the pool's own shape; None stands for the pool's own value.

What the shapes cover: 65 (first beyond the long kernel), 66 / 72 / 80 (a second EVSE tile, short), 130 (a third tile), 257,
512, 1,024 (the last tile full); K = 4 with pinned variables; both cones; a peak row, scalar, vector and unlimited; an
infeasible instance the final check rejects; horizon 48 (strips of 12 periods) and horizons that are no multiple of 4."""
import functools

import numpy as np

from tests import polish_cases as PC
from tests import polish_long_cases as LC

CHECK_EVERY = PC.CHECK_EVERY
WINDOW = PC.WINDOW
LATE = dict(max_iter=800, eps_abs=1e-30, eps_rel=1e-30)

POOLS = {
    "n65_soc": lambda: PC.site_pool((65, 4, 0.5), "SOC", (8, 6, 7), 6, 81, two=False),
    "n72_lin_multi": lambda: PC.site_pool((72, 4, 0.9), "LINEAR", (12, 10, 9), 4, 84, multi=True),
    "n72_soc_multi": lambda: PC.site_pool((72, 4, 0.9), "SOC", (12, 10, 9), 4, 84, multi=True),
    "n80_lin_peak": lambda: PC.site_pool((80, 4, 0.4), "LINEAR", (12, 9, 10), 6, 82, two=False, peak="mixed", peak_range=(300, 700)),
    "n66_soc_t48": lambda: PC.site_pool((66, 4, 0.5), "SOC", (48, 40, 33), 3, 85, two=False),
    "n130_soc": lambda: PC.site_pool((130, 6, 0.5), "SOC", (6, 5), 4, 83),
    "n257_soc_rounds": lambda: PC.site_pool((257, 8, 0.5), "SOC", (5, 4), 3, 86, two=False),
    "n512_soc_late": lambda: PC.site_pool((512, 8, 0.6), "SOC", (8, 6), 2, 89, two=False),
    "n1024_soc_late": lambda: PC.site_pool((1024, 16, 0.9), "SOC", (3,), 2, 87, two=False),
}

CASES = {
    "n65_soc": ("n65_soc", dict(max_iter=100), ((17, None), (None, 4)), False, (4, 4, 13, {})),
    "n72_lin_multi": ("n72_lin_multi", dict(max_iter=100), (), False, (4, 4, 16, {})),
    "n72_soc_multi": ("n72_soc_multi", dict(max_iter=100), (), False, (4, 4, 16, {})),
    "n80_lin_peak": ("n80_lin_peak", dict(max_iter=60), ((33, None),), False, (6, 5, WINDOW, {"verify": 1})),
    "n66_soc_t48": ("n66_soc_t48", dict(max_iter=100), (), False, (3, 3, 16, {})),
    "n130_soc": ("n130_soc", dict(max_iter=100), (), False, (4, 4, 27, {})),
    "n257_soc_rounds": ("n257_soc_rounds", dict(max_iter=100), (), False, (3, 0, 0, {"rounds": 3})),
    "n512_soc_late": ("n512_soc_late", LATE, (), True, (2, 2, 2, {})),
    "n1024_soc_late": ("n1024_soc_late", LATE, (), True, (2, 2, 3, {})),
}


@functools.lru_cache(maxsize=None)
def pool(name):
    return POOLS[name]()


def shapes(case):
    """the padded shapes (t_max, K) a case is launched at: its own first"""
    p = pool(CASES[case][0])
    out = [(p.Tm, p.K)]
    for t, k in CASES[case][2]:
        s = (p.Tm if t is None else t, p.K if k is None else k)
        if s[0] >= p.Tm and s[1] >= p.K and s not in out:
            out.append(s)
    return out


def start_options(case):
    """the options of the launch whose end is the hand-over point: the case's start and no retry pass"""
    return dict(CASES[case][1], retry_passes=0)


@functools.lru_cache(maxsize=None)
def twin(name, start=None):
    """oracle/admm_port of the pool with the kernels' Anderson columns and no retry pass: stopped by the start options
    (a sorted tuple of items), or the full solve"""
    from oracle import admm_port

    kw = dict(accel_mem=5, retry_passes=0)
    kw.update(dict(start or ()))
    out = admm_port.solve_batch(pool(name), threads=min(8, admm_port.max_threads()), **kw)
    for a in out.values():
        a.setflags(write=False)
    return out


def spec_job(batch, b, x0, y0, t_max=None):
    return (LC.worst_rows(batch.site, batch.Tm if t_max is None else t_max), PC.spec_args(batch, b, x0, y0))


spec_many = LC.spec_many


@functools.lru_cache(maxsize=None)
def cpu_case(case):
    """from the twin's last iterate under the start options: dict(index: problems it ended MAX_ITER or SOLVED_INACCURATE,
    spec: {b: (x, info)}, final: the twin's full solve)"""
    name, start = CASES[case][:2]
    batch, at, final = pool(name), twin(name, tuple(sorted(start.items()))), twin(name)
    index = [int(b) for b in np.flatnonzero(np.isin(at["status"], (2, 5)))]
    res = spec_many([spec_job(batch, b, at["x"][b], at["y"][b]) for b in index])
    return dict(index=index, spec=dict(zip(index, res)), final=final, at=at)
