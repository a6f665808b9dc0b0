"""The polish kernel's pools, stated once: tests/test_polish_cases.py proves on the CPU that they are fit for the job (enough
problems handed over, the specification accepts them, the give-up pools give up for the stated reason) and
tests/test_polish_gpu.py holds ``polish_kernel<4 | 8>`` (adacharge_amd/csrc/acn_qp_polish.hpp) to oracle/polish_ref.py on them,
problem by problem.  A plain module, like warm_cases.py; nothing at import time but numpy, so that the worker processes of
``spec_many`` (the specification is a Python loop: 50 ms a round at N = 54) never load the library.

A case is a pool and a hand-over iteration P (a multiple of check_every = 20).  ``expect`` says what the case is for:
  accept      the specification accepts at least three quarters of the feasible problems that are not SOLVED at P
  rounds      ... and some run out of the 96 rounds                      (gave_up_rounds)
  rows        the iterate at P has more tight rows than the row tables hold: the solver declines the hand-over
  verify      the final check rejects the point the polish reaches       (gave_up_kkt; the N = 3 site)
``late`` cases (P >= 100: the working set at P is nearly right) also pin the round count outside ROUND_FRAGILE."""
import functools

import numpy as np

SEED = 20250
CHECK_EVERY = 20
T_PADS = (13, 16, 17, 29, 32)      # with the pool's own Tm: both instantiations, TQ = 4, 4, 5, 8, 8 with a short last quarter
K_PADS = (4,)                      # with the pool's own K
WINDOW = 96                        # Newton rounds at most (polish_ref.MAX_ROUNDS)


def _infra(site):
    from adacharge_amd import sites

    if isinstance(site, str):
        return getattr(sites, site)()
    n, pods, frac = site
    return sites.balanced_three_phase(n, pods, frac, name=f"B{n}")


def _multi_sessions(infra, T, rng):
    """three or four real sessions with disjoint windows on a third of the EVSEs, one elsewhere; minimum rates over a prefix
    (lb > 0), a stepped maximum, and a fifth of the sessions with one period pinned (lb == ub == 6 A)"""
    from adacharge_amd.acn import SessionInfo

    out = []
    n = infra.num_stations
    for i in rng.choice(n, size=int(rng.integers(n // 2, n + 1)), replace=False):
        sid = infra.station_ids[int(i)]
        k = float(infra.voltages[int(i)]) * 5 / 60 / 1e3
        parts = int(rng.integers(3, 5)) if rng.random() < 0.34 else 1
        cuts = np.r_[0, np.sort(rng.choice(np.arange(2, T - 1), size=parts - 1, replace=False)), T] if parts > 1 else np.array([int(rng.integers(0, T // 3)), T])
        for j in range(len(cuts) - 1):
            a, d = int(cuts[j]), int(cuts[j + 1])
            if parts > 1 and d - a > 2 and rng.random() < 0.5:
                d -= 1                                       # a gap between two windows
            L = d - a
            mins, maxs = np.zeros(L), np.full(L, 32.0)
            if rng.random() < 0.3:
                mins[: int(rng.integers(1, L + 1))] = 6.0
            if rng.random() < 0.2:
                maxs[int(rng.integers(0, L)):] = 16.0
            if rng.random() < 0.2:
                p = int(rng.integers(0, L))
                mins[p] = maxs[p] = 6.0
            dem = max(float(rng.uniform(0.2, 1.0) * 1.5 * 32 * L * k), mins.sum() * k + 0.01)
            out.append(SessionInfo(sid, f"{sid}-{j}", dem, 0.0, a, d, current_time=0, min_rates=mins, max_rates=maxs))
    return out


def site_pool(site, cone, horizons, n, seed, eq=False, two=True, peak=None, peak_range=(250.0, 600.0), min_rates=None,
              demand_scale=None, multi=False):
    """helpers.certificate_pool for any site: ``n`` snapshots of sites.random_sessions_general (``multi``: _multi_sessions),
    horizons ``horizons[k % len]``; ``peak``: None, "scalar", "vector" or "mixed" (scalar, vector, unlimited in turn)."""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites, total_energy
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch

    infra = _infra(site)
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(seed)
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3), ObjectiveComponent(total_energy, 0.5)]
    snaps, peaks = [], []
    for k in range(n):
        Tb = horizons[k % len(horizons)]
        if multi:
            snaps.append(_multi_sessions(infra, Tb, rng))
        else:
            snaps.append(sites.random_sessions_general(infra, Tb, rng, two_per_evse=two, min_rates=(not eq) if min_rates is None else min_rates,
                                                       demand_scale=(0.5 if eq else 1.5) if demand_scale is None else demand_scale))
        kind = peak if peak != "mixed" else ("scalar", "vector", None)[k % 3]
        Tk = max(s.arrival_offset + s.remaining_time for s in snaps[-1])
        peaks.append(None if kind is None else float(rng.uniform(*peak_range)) if kind == "scalar" else rng.uniform(*peak_range, size=Tk))
    return build_batch(snaps, infra, iface, obj, cone, eq, peak_limits=peaks if peak else None)


N64 = (64, 4, 0.4)
POOLS = {
    "ct54_soc_two": lambda: site_pool("caltech54", "SOC", (12, 10, 8), 24, 51),
    "ct54_lin_eq_peak": lambda: site_pool("caltech54", "LINEAR", (12, 10, 8), 24, 52, eq=True, peak="mixed"),
    "ct54_soc_t24_peak": lambda: site_pool("caltech54", "SOC", (24, 22, 20), 16, 53, peak="mixed"),
    "ct54_soc_multi": lambda: site_pool("caltech54", "SOC", (12, 10, 8), 24, 55, multi=True),
    "jpl_soc_t17": lambda: site_pool("jpl52", "SOC", (17, 15, 13), 8, 56),
    "n64_lin_t16_peak": lambda: site_pool(N64, "LINEAR", (16, 14, 12), 24, 57, peak="scalar", peak_range=(700.0, 700.0)),
    "jpl_soc_t32_rows": lambda: site_pool("jpl52", "SOC", (32, 30, 28), 8, 58),
    "jpl_soc_t32": lambda: site_pool((52, 4, 0.8), "SOC", (32, 30, 28), 16, 59),
    "n8_soc": lambda: site_pool((8, 1, 0.5), "SOC", (5, 4, 3), 24, 3, two=False, min_rates=True, demand_scale=1.5),
    "n3_soc": lambda: site_pool((3, 1, 0.5), "SOC", (5, 4, 3), 24, 3, two=False, min_rates=True, demand_scale=1.5),
    "ct54_soc_peak_one": lambda: site_pool("caltech54", "SOC", (12, 10, 8), 24, 60, two=False, peak="mixed"),
    "jpl_soc_t12_one": lambda: site_pool("jpl52", "SOC", (12, 10, 8), 16, 61, two=False),
}


# case -> (pool, P, expect, late).  Measured on the CPU from the twin's iterate (tests/test_polish_cases.py holds every line):
# problems not SOLVED at P / accepted by the specification / rounds at most among the accepted.
CASES = {
    "ct54_soc_two@40": ("ct54_soc_two", 40, "accept", False),            # 12 / 12 / 31: K = 2, lb > 0, stepped ub
    "ct54_soc_two@100": ("ct54_soc_two", 100, "accept", True),           # 10 / 10 / 33
    "ct54_lin_eq_peak@20": ("ct54_lin_eq_peak", 20, "accept", False),    # 22 / 21 / 73, one infeasible: box rows, equalities,
    "ct54_lin_eq_peak@100": ("ct54_lin_eq_peak", 100, "accept", True),   # 17 / 16 / 14   scalar, vector and no peak in one batch
    "ct54_soc_multi@40": ("ct54_soc_multi", 40, "accept", False),        # 21 / 21 / 75: three and four sessions, lb == ub
    "ct54_soc_t24_peak@100": ("ct54_soc_t24_peak", 100, "accept", True),  # 11 / 11 / 12: polish_kernel<8>, discs and a peak row
    "jpl_soc_t17@40": ("jpl_soc_t17", 40, "rounds", False),              # 8 / 5, three run out of rounds: two row tiles
    "jpl_soc_t17@100": ("jpl_soc_t17", 100, "accept", True),             # 8 / 8 / 69
    "n64_lin_t16_peak@100": ("n64_lin_t16_peak", 100, "accept", True),   # 24 / 20 / 27, four infeasible: all 256 threads own variables
    "jpl_soc_t32_rows@40": ("jpl_soc_t32_rows", 40, "rows", False),      # 8, four declined with 318 ... 380 rows
    "jpl_soc_t32@100": ("jpl_soc_t32", 100, "accept", True),             # 16 / 15 / 50: polish_kernel<8> over all 32 periods
    "ct54_soc_peak_one@20": ("ct54_soc_peak_one", 20, "accept", False),  # 20 / 20 / 65: K = 1 with a peak row: the wave routes
    "ct54_soc_peak_one@100": ("ct54_soc_peak_one", 100, "accept", True),  # 19 / 19 / 30
    "jpl_soc_t12_one@200": ("jpl_soc_t12_one", 200, "accept", True),     # 16 / 16 / 15: K = 1, two row tiles
    "n8_soc@40": ("n8_soc", 40, "accept", False),                        # 24 / 24 / 43
    "n3_soc@40": ("n3_soc", 40, "verify", False),                        # 24: 10 accepted, 9 rejected by the final check
}


@functools.lru_cache(maxsize=None)
def pool(name):
    return POOLS[name]()


# ---- the twin ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin(name, P=None, eps=None):
    """oracle/admm_port of the pool with the kernels' Anderson columns and no retry pass: the iterate at ``P`` (what a solver
    kernel hands over), or the full solve (``eps``: eps_abs = eps_rel)"""
    from oracle import admm_port

    kw = dict(accel_mem=5, retry_passes=0)
    if P is not None:
        kw["max_iter"] = int(P)
    if eps is not None:
        kw["eps_abs"] = kw["eps_rel"] = eps
    out = admm_port.solve_batch(pool(name), threads=min(8, admm_port.max_threads()), **kw)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the specification, in worker processes -----------------------------------------------------------------------------
def spec_args(batch, b, x0, y0, reg_rel=0.06):
    """arguments of polish_ref.polish for problem ``b`` (what polish_ref.polish_batch_problem builds), as plain arrays"""
    from oracle.polish_ref import effective_pdiag

    site = batch.site
    T = int(batch.T[b])
    lb, q = np.array(batch.lb[b][:, :T], float), np.array(batch.q[b][:, :T], float)
    ub = np.maximum(batch.ub[b][:, :T], lb)
    sessions = []
    for k in range(batch.K):
        for i in range(site.N):
            L = int(batch.s_len[b, k, i])
            if L:
                sessions.append((i, int(batch.s_off[b, k, i]), L, float(batch.s_cap[b, k, i]), k))
    pd = effective_pdiag(float(batch.pdiag[b]), reg_rel, float(np.abs(q).max()), float(ub.max()), T)
    peak = None if batch.peak is None else np.asarray(batch.peak[b][:T], float)
    return (lb, ub, q, pd, sessions, bool(batch.s_eq[b]), np.asarray(site.G, float), int(site.M), int(site.cone) == 1,
            np.asarray(site.limits, float), peak, np.array(np.asarray(x0, float)[:, :T]), np.array(np.asarray(y0, float)[:, :T]))


def _spec_one(args):
    from oracle.polish_ref import polish

    x, info = polish(*args)
    return x, info


_CACHE = {}


def spec_many(jobs):
    """[(x, info)] of polish_ref.polish for a list of spec_args tuples; equal arguments are run once (a dict keyed by the
    arguments' bytes), the rest in up to eight fresh worker processes that import numpy and the specification alone"""
    import hashlib
    import os
    import pickle
    import subprocess
    import sys
    import tempfile

    keys = [hashlib.sha1(pickle.dumps(j, protocol=4)).digest() for j in jobs]
    todo = {k: j for k, j in zip(keys, jobs) if k not in _CACHE}
    if len(todo) <= 2:
        for k, j in todo.items():
            _CACHE[k] = _spec_one(j)
    else:
        n = min(8, os.cpu_count() or 1, len(todo))
        items = list(todo.items())
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        # (a Python loop over small matrices: one BLAS thread per worker, not the machine's default times eight)
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
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


def perturbed(x0, y0, rel, seed):
    """the start point moved by ``rel`` relative, entry by entry"""
    r = np.random.default_rng([SEED, seed])
    return x0 * (1.0 + rel * r.standard_normal(x0.shape)), y0 * (1.0 + rel * r.standard_normal(y0.shape))


def declined_rows(batch, b, y, t_max):
    """DESIGN.md 2.3, acn_qp_check.hpp: the rows the polish's Schur system would have, counted from the site-row multipliers
    at the hand-over (two per tight disc, one per tight box or peak row; tight: multiplier, in the solver's row scaling, above
    1e-9 max(1, |q|_inf)); the hand-over is declined when count + 8 exceeds the row tables of the padded shape"""
    from oracle import admm_port

    site = batch.site
    admm_port.equilibrated(site)
    scale = admm_port.equilibrated.last_scale
    T = int(batch.T[b])
    ys = np.asarray(y, float)[:, :T] / scale[:, None]
    tol = 1e-9 * max(1.0, float(np.abs(batch.q[b]).max()))
    M, soc = int(site.M), int(site.cone) == 1
    cnt = 2 * int((np.hypot(ys[:M], ys[M:2 * M]) > tol).sum()) if soc else int((ys[:M] > tol).sum())
    if site.has_peak:
        cnt += int((ys[site.Mg - 1] > tol).sum())
    nrow = M + int(bool(site.has_peak))
    return cnt, cnt + 8 > min(256, ((2 * nrow * t_max + 7) // 8) * 8)


def polish_tables(site, t_max, k, tiled):
    """(rows, session columns, doubles for the packed per-period blocks) the polish kernel's LDS holds at a padded shape --
    polish_max_rows, polish_max_sess and PolishLds of acn_qp_pollds.hpp with the LDS budget of polish_plan
    (acn_qp_polplan.hpp), restated; blocks -1: not even one full block fits and the library runs no polish at this shape.
    ``tiled``: the route is one of the register-resident families (two workgroups per CU at t_max <= 16, one row tile, one
    session slot).  tests/test_polish_plan.py compiles the two headers for the host and holds this restatement to them on
    the CPU, shape by shape; tests/test_polish_gpu.py holds it to what the library runs."""
    N, M, Mg, soc, pk = int(site.N), int(site.M), int(site.Mg), int(site.cone) == 1, int(bool(site.has_peak))
    nrow = M + pk
    rows = min(256, ((2 * nrow * t_max + 7) // 8) * 8)
    sess = min(128, ((N * k + 7) // 8) * 8)
    padded = (8 * ((M + 3) // 4) if soc else M) + pk
    two_per_cu = tiled and t_max <= 16 and max(16, 16 * ((padded + 15) // 16)) == 16 and k == 1
    lds = min(76 * 1024 if two_per_cu else 160 * 1024, 160 * 1024 - 2048)
    fixed = (2 * N * t_max + Mg * N + 2 * Mg * t_max + nrow * t_max + 4 * N + 5 * rows + sess * (sess + 1) // 2 + 2 * nrow * sess
             + 2 * sess + 16)
    nint = 3 * rows + 2 * (t_max + 1) + nrow + 8 + 2 * sess
    fixed += (nint + 1) // 2 + (N * t_max + 7) // 8
    room = (lds - 8 * fixed) // 8
    blocks = max(0, min(room, t_max * (2 * nrow) * (2 * nrow + 1) // 2))
    return rows, sess, (blocks if blocks >= 2 * nrow * (2 * nrow + 1) // 2 else -1)


def outgrows(info, tables):
    """the kernel gives this problem up for `rows` in the round whose blocks or session columns its tables do not hold"""
    return info.get("sessions", 0) > tables[1] or info.get("blocks", 0) > tables[2]


FRAGILE_REL = 1e-9      # the perturbation of (x0, y0) that defines ROUND_FRAGILE
FRAGILE_SEEDS = (1, 2, 3)


def fragile_of(batch, index, points, base, rel=FRAGILE_REL):
    """the problems ``index`` whose verdict or round count moves when the start point ``points[n]`` = (x0, y0) moves by ``rel``
    relative (three draws); ``base``: [(x, info)] from the points themselves"""
    jobs = [spec_args(batch, b, *perturbed(x0, y0, rel, seed)) for seed in FRAGILE_SEEDS for b, (x0, y0) in zip(index, points)]
    res = spec_many(jobs)
    out = []
    for n, b in enumerate(index):
        info = base[n][1]
        moved = any((r[1]["ok"], r[1]["why"], r[1]["rounds"]) != (info["ok"], info["why"], info["rounds"]) for r in res[n::len(index)])
        if moved:
            out.append(int(b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cpu_case(case):
    """from the twin's iterate at P: dict(index: problems not SOLVED there, declined: those the solver would not hand over at
    the pool's own shape, spec: {b: (x, info)} of the others, fragile: tuple, final: the twin's full solve)"""
    name, P, _, _ = CASES[case]
    batch, at, final = pool(name), twin(name, P), twin(name)
    index = [int(b) for b in np.flatnonzero(at["status"] != 1)]
    declined = [b for b in index if declined_rows(batch, b, at["y"][b], batch.Tm)[1]]
    run = [b for b in index if b not in declined]
    points = [(at["x"][b], at["y"][b]) for b in run]
    res = spec_many([spec_args(batch, b, *pt) for b, pt in zip(run, points)])
    # (a `rows` case is there for what the solver declines: no set of its own, so nothing excuses a disagreement on the rest)
    fragile = () if CASES[case][2] == "rows" else fragile_of(batch, run, points, res)
    return dict(index=index, declined=declined, spec=dict(zip(run, res)), fragile=fragile, final=final)


# measured by cpu_case (tests/test_polish_cases.py holds them): the problems whose verdict or round count moves with the
# start point at FRAGILE_REL.  (At 1e-12 relative three problems fewer -- ct54_soc_two@40 21, jpl_soc_t17@100 0, jpl_soc_t32@100 14;
# the second, a 69-round polish, the kernel ends three rounds later than the specification with the same answer: the 1e-9
# the regularised solve's rounding asks for.)  The sets are RECORDED: they hang on the last bits of the specification's
# arithmetic, so another numpy or BLAS build may move one -- the CPU test then prints the set it finds, to be recorded here
# again; what must hold of any such set is asserted apart from its members (below half of a late case).
ROUND_FRAGILE = {
    "ct54_soc_two@40": (2, 3, 21),
    "ct54_soc_two@100": (2,),
    "ct54_soc_multi@40": (9, 14, 17),
    "ct54_soc_t24_peak@100": (14,),
    "jpl_soc_t17@40": (7,),
    "jpl_soc_t17@100": (0, 3),
    "jpl_soc_t32@100": (14,),
    "ct54_soc_peak_one@20": (0,),
    "ct54_soc_peak_one@100": (0,),
    "jpl_soc_t12_one@200": (9,),
    "n8_soc@40": (0, 3, 4, 5, 6, 8, 9, 10, 11, 13, 14, 17, 20, 21, 22),
    "n3_soc@40": (0, 5),
}


def solve_case(case, t_max, k):
    """the polished launch of a case at a padded shape (device entry, multipliers wanted) under the environment of this
    process, with what acnqp_debug_polish_alongside and the polish counters say about it"""
    import torch

    from adacharge_amd.backend import DeviceBatch, SiteHandle, default_options
    from tests import helpers as H

    name, P, _, _ = CASES[case]
    padded = H.pad_batch(pool(name), t_max, k)
    h = SiteHandle(padded.site, 0)
    h.polish_alongside()
    before = h.polish_stats()
    dev = DeviceBatch(padded, "cuda:0", want_y=True)
    h.solve_device(dev, default_options(polish_iters=P, retry_passes=0), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = H.device_outputs(dev)
    out["alongside"] = h.polish_alongside()
    after = h.polish_stats()
    out["attempted"], out["solved"] = after["attempted"] - before["attempted"], after["solved"] - before["solved"]
    out["family"] = h.route(t_max, k, padded.B)[0]
    h.close()
    return out


if __name__ == "__main__":   # a worker of spec_many: jobs in, (x, info) out; or ``--solve CASE T_MAX K OUT.npz``
    import os
    import pickle
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--solve":
        from tests import polish_cases as _self   # (the pools' caches live in the imported module)

        np.savez_compressed(sys.argv[5], **_self.solve_case(sys.argv[2], int(sys.argv[3]), int(sys.argv[4])))
        sys.exit(0)
    with open(sys.argv[1], "rb") as f:
        todo = pickle.load(f)
    with open(sys.argv[2], "wb") as f:
        pickle.dump([_spec_one(j) for j in todo], f, protocol=4)
