"""The long-horizon polish kernel's pools (adacharge_amd/csrc/acn_qp_polish_long.hpp: horizons 33 ... 288, N <= 64), stated
once: tests/test_polish_long_cases.py proves on the CPU that they are fit for the job and tests/test_polish_long_gpu.py holds
the kernel to oracle/polish_ref.py on them, problem by problem.  The pools are tests.polish_cases.site_pool's; a plain module
like that one (nothing at import time but numpy), with a worker of its own: the specification's module constant MAX_ROWS
(256, the short kernel's row tables) is raised to the worst-case row count of the shape before ``polish`` is called --
the long kernel's tables hold every site row tight in every period with its tangent row, so nothing is ever given up for
`rows`.  MAX_ROUNDS = 96 stays.

A case is a pool, a hand-over iteration P (a multiple of check_every = 20) and the padded shapes it is launched at.
``expect``:
  accept      the specification accepts at least three quarters of the feasible problems that are not SOLVED at P
  rounds      ... and some run out of the 96 rounds
``late`` cases (P >= 100) also pin the round count.

What the shapes cover: 33 (first beyond the short kernel), 48 and 49 (wave5 | long_ws), 65 (past one 64-bit word of
periods), >= 257 (past the 8 bits pol_code gives a period), a short last strip (Tm % 4 != 0), K = 4, pinned variables
(lb == ub: the equalities of the multi-session pool), scalar and vector peak, both cones."""
import functools

import numpy as np

from tests import polish_cases as PC

CHECK_EVERY = PC.CHECK_EVERY
WINDOW = PC.WINDOW
N8 = (8, 1, 0.5)
B52 = (52, 4, 0.8)

POOLS = {
    "n8_t144": lambda: PC.site_pool(N8, "SOC", (144, 100, 65), 4, 71, two=False, min_rates=True, demand_scale=1.5),
    "ct54_t48": lambda: PC.site_pool("caltech54", "SOC", (48, 36, 33), 6, 75, two=False),
    "ct54_t48_peak": lambda: PC.site_pool("caltech54", "SOC", (36, 33, 48), 3, 72, two=False, peak="mixed"),
    "ct54_lin_multi": lambda: PC.site_pool("caltech54", "LINEAR", (40, 37, 34), 4, 76, multi=True),
    "b52_t48_two": lambda: PC.site_pool(B52, "SOC", (48, 40, 33), 3, 74),
    "n64_lin_t96_peak": lambda: PC.site_pool(PC.N64, "LINEAR", (65, 70, 96), 4, 77, peak="scalar", peak_range=(700.0, 700.0)),
    "b52_t144": lambda: PC.site_pool(B52, "SOC", (144, 96), 2, 78),
    "n8_t288": lambda: PC.site_pool(N8, "SOC", (288, 260), 2, 79, two=False, min_rates=True, demand_scale=1.5),
}

# case -> (pool, P, expect, late, pads).  Measured on the CPU from the twin's iterate (tests/test_polish_long_cases.py holds
# every line).  pads: (t_max, K) beyond the pool's own shape; None stands for the pool's own value.
CASES = {
    "n8_t144@100": ("n8_t144", 100, "accept", True, ()),                       # Tm 139: 4 / 4, 44 rounds at most
    "ct54_t48@40": ("ct54_t48", 40, "accept", False, ((49, None), (None, 4))),  # 6 / 6, <= 16 rounds: wave5, long_ws by t_max and by K
    "ct54_t48_peak@40": ("ct54_t48_peak", 40, "accept", False, ((49, None),)),  # 3 / 3, <= 70 rounds: 17 site rows, two row tiles
    "ct54_lin_multi@40": ("ct54_lin_multi", 40, "accept", False, ((49, None),)),  # 4 / 4, <= 30 rounds: K = 4, lb == ub
    "b52_t48_two@100": ("b52_t48_two", 100, "accept", True, ((49, None),)),     # 2 / 2 open, 3 rounds: K = 2
    "n64_lin_t96_peak@60": ("n64_lin_t96_peak", 60, "accept", False, ()),       # 3 accepted, the infeasible fourth runs out of rounds
    "b52_t144@60": ("b52_t144", 60, "rounds", False, ()),                       # T = 96 accepted in 6 rounds, T = 144 runs out of 96
    "n8_t288@100": ("n8_t288", 100, "accept", True, ((288, None),)),            # Tm 274: 2 / 2, <= 4 rounds; a period index >= 256
}


@functools.lru_cache(maxsize=None)
def pool(name):
    return POOLS[name]()


def shapes(case):
    """the padded shapes (t_max, K) a case is launched at: its own first"""
    p = pool(CASES[case][0])
    out = [(p.Tm, p.K)]
    for t, k in CASES[case][4]:
        s = (p.Tm if t is None else t, p.K if k is None else k)
        if s[0] >= p.Tm and s[1] >= p.K and s not in out:
            out.append(s)
    return out


def worst_rows(site, t_max):
    """rows of the Schur system at most at a shape: every site row tight in every period with its tangent row (two per disc,
    one per box or peak row: the ABI's row count) -- polish_long_rows of acn_qp_polslab.hpp, restated"""
    return int(site.Mg) * int(t_max)


@functools.lru_cache(maxsize=None)
def twin(name, P=None):
    """oracle/admm_port of the pool with the kernels' Anderson columns and no retry pass: the iterate at ``P`` or the full solve"""
    from oracle import admm_port

    kw = dict(accel_mem=5, retry_passes=0)
    if P is not None:
        kw["max_iter"] = int(P)
    out = admm_port.solve_batch(pool(name), threads=min(8, admm_port.max_threads()), **kw)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the specification with the long kernel's row tables, in worker processes ------------------------------------------------
def _spec_one(job):
    from oracle import polish_ref

    max_rows, args = job
    polish_ref.MAX_ROWS = int(max_rows)   # (a module constant read at every round; oracle/polish_ref.py itself is not edited)
    return polish_ref.polish(*args)


_CACHE = {}


def spec_many(jobs):
    """[(x, info)] of polish_ref.polish for a list of (max_rows, spec_args) jobs; equal jobs are run once, the rest in up to
    eight fresh worker processes that import numpy and the specification alone (polish_cases.spec_many's scheme)"""
    import hashlib
    import os
    import pickle
    import subprocess
    import sys
    import tempfile

    keys = [hashlib.sha1(pickle.dumps(j, protocol=4)).digest() for j in jobs]
    todo = {k: j for k, j in zip(keys, jobs) if k not in _CACHE}
    if todo:
        n = min(8, os.cpu_count() or 1, len(todo))
        items = list(todo.items())
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1",
                   PYTHONPATH=os.pathsep.join([root] + [p for p in (os.environ.get("PYTHONPATH"),) if p]))
        with tempfile.TemporaryDirectory() as tmp:
            procs = []
            for w in range(n):
                with open(os.path.join(tmp, f"in{w}.pkl"), "wb") as f:
                    pickle.dump([j for _, j in items[w::n]], f, protocol=4)
                procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), os.path.join(tmp, f"in{w}.pkl"),
                                               os.path.join(tmp, f"out{w}.pkl")], cwd=root, env=env))
            codes = [p.wait() for p in procs]
            assert not any(codes), codes
            for w in range(n):
                with open(os.path.join(tmp, f"out{w}.pkl"), "rb") as f:
                    for (k, _), res in zip(items[w::n], pickle.load(f)):
                        _CACHE[k] = res
    return [_CACHE[k] for k in keys]


def spec_job(batch, b, x0, y0):
    return (worst_rows(batch.site, batch.Tm), PC.spec_args(batch, b, x0, y0))


@functools.lru_cache(maxsize=None)
def cpu_case(case):
    """from the twin's iterate at P: dict(index: problems not SOLVED there, spec: {b: (x, info)}, final: the twin's full solve)"""
    name, P = CASES[case][:2]
    batch, at, final = pool(name), twin(name, P), twin(name)
    index = [int(b) for b in np.flatnonzero(at["status"] != 1)]
    res = spec_many([spec_job(batch, b, at["x"][b], at["y"][b]) for b in index])
    return dict(index=index, spec=dict(zip(index, res)), final=final)


if __name__ == "__main__":   # a worker of spec_many: jobs in, (x, info) out
    import pickle
    import sys

    with open(sys.argv[1], "rb") as f:
        todo = pickle.load(f)
    with open(sys.argv[2], "wb") as f:
        pickle.dump([_spec_one(j) for j in todo], f, protocol=4)
