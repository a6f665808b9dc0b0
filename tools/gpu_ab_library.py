"""Bitwise A/B of two builds of libacn_qp_hip.so on the pools of the route-certificate and verdict tests: the pools of
tests/test_route_certificate.py (all eleven kernel families and the polish) and of tests/test_verdicts_gpu.py (every
probe, both sides of the boundary, and the max_iter = check_every = 20 runs), each padded to every family it reaches
and launched through the device entry with every output poisoned.  x, y, status, iters, pri_res, dua_res and obj must
agree BIT FOR BIT between the two libraries.  The `warm` group feeds the one input those pools leave out: the pools of
tests/warm_cases.py on every family they reach, from every kind of warm point after 60 plain iterations and from the
perturbed point as shipped.  One child process per library and pool group (ACNQP_LIBRARY selects the
library), one at a time, each under its own time limit; the first non-zero exit ends the run.
The `polish` and `polish_long` groups hand work to the Newton polish on purpose: every case of tests/polish_cases.py at its
pool's own shape (and at t_max = 17 where the pool's is <= 16: polish_kernel<4> becomes <8> there) and every case of
tests/polish_long_cases.py at its shapes on a polish_long handle, with polish_iters = the case's hand-over point and no
retry passes; besides the outputs, what each launch adds to the polish counters (attempted, solved, the four give-up
reasons, rounds) must be equal.

    python tools/gpu_ab_library.py child <group> <out.npz>          one library (ACNQP_LIBRARY), one group of pools
    python tools/gpu_ab_library.py <other.so> [record.json]         both libraries, compared; the record holds the
                                                                    arrays compared, the mismatches and both sha256"""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

KEYS = ("x", "y", "status", "iters", "pri_res", "dua_res", "obj")
GROUPS = ("routes", "verdicts_a", "verdicts_b", "max_iter", "warm", "polish", "polish_long")
POLISH_COUNTERS = ("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt", "rounds")
CHILD_TIMEOUT = 900   # seconds per child


def runs(group):
    """(tag, handle, padded batch, options, warm point or None) of every launch of the group"""
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import ProblemBatch
    from tests import helpers as H
    from tests import test_route_certificate as R
    from tests import test_verdicts_gpu as G

    if group == "routes":
        for name in R.POOLS:
            pool = R.POOLS[name]()
            h = SiteHandle(pool.site, 0)
            for fam, (t, k) in H.route_shapes(h, pool).items():
                yield f"route/{name}/{fam}", h, H.pad_batch(pool, t, k), None, None
            h.close()
    elif group in ("verdicts_a", "verdicts_b"):
        names = list(G.POOLS)
        for name in names[:len(names) // 2] if group == "verdicts_a" else names[len(names) // 2:]:
            _, pool = G._pool(name)
            h = SiteHandle(pool.site, 0)
            for fam, (t, k) in H.route_shapes(h, pool).items():
                if G.POOLS[name]["want"] is None or fam in G.POOLS[name]["want"]:
                    yield f"verdict/{name}/{fam}", h, H.pad_batch(pool, t, k), None, None
            h.close()
    elif group == "warm":
        from tests import warm_cases as WC

        for name, want in WC.POOLS.items():
            pool = WC.pool(name)
            h = SiteHandle(pool.site, 0)
            for fam, (t, k) in H.route_shapes(h, pool).items():
                if want is None or fam in want:
                    for kind, run in [(kind, "m60") for kind in WC.kinds_of(name, t)] + [("perturbed", "shipped")]:
                        yield f"warm/{name}/{fam}/{kind}/{run}", h, H.pad_batch(pool, t, k), default_options(**WC.RUNS[run]), WC.warm(name, kind, t)
            h.close()
    elif group == "polish":
        from tests import polish_cases as PC

        for case, (name, P, *_) in PC.CASES.items():
            pool = PC.pool(name)
            h = SiteHandle(pool.site, 0)
            for t in [pool.Tm] + ([17] if pool.Tm <= 16 else []):
                yield f"polish/{case}/t{t}", h, H.pad_batch(pool, t, pool.K), default_options(polish_iters=P, retry_passes=0), None
            h.close()
    elif group == "polish_long":
        from tests import polish_long_cases as LC

        for case, (name, P, *_) in LC.CASES.items():
            pool = LC.pool(name)
            h = SiteHandle(pool.site, 0, polish_long=True)
            for t, k in LC.shapes(case):
                yield f"polish_long/{case}/t{t}k{k}", h, H.pad_batch(pool, t, k), default_options(polish_iters=P, retry_passes=0), None
            h.close()
    else:
        for name in G.MAX_ITER_POOLS:
            pool = ProblemBatch.concatenate(G._filler(G.POOLS[name], np.random.default_rng(77), 24))
            h = SiteHandle(pool.site, 0)
            for fam, (t, k) in H.route_shapes(h, pool).items():
                yield f"max_iter/{name}/{fam}", h, H.pad_batch(pool, t, k), default_options(max_iter=20, check_every=20), None
            h.close()


def child(group, path):
    from tests import helpers as H

    res = {}
    for tag, h, padded, opts, warm in runs(group):
        s0 = h.polish_stats() if group.startswith("polish") else None
        out = H.launch_poisoned(h, padded, opts, warm=warm)
        for k in KEYS:
            res[f"{tag}/{k}"] = out[k]
        if s0 is not None:
            s1 = h.polish_stats()
            res[f"{tag}/polish_counters"] = np.array([s1[c] - s0[c] for c in POLISH_COUNTERS], np.int64)
    np.savez(path, **res)


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
        raise SystemExit(0)
    from adacharge_amd.build import LIB

    other = os.path.abspath(sys.argv[1])
    record = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r05_ab_library.json")
    outdir = tempfile.mkdtemp(prefix="acnqp_ab_")   # the children's arrays: tens of MB per group, removed once compared
    arrays, mismatches, statuses = [], [], {}
    for group in GROUPS:
        files = []
        for tag, lib in (("this", None), ("other", other)):
            env = dict(os.environ)
            env["ACNQP_LIBRARY"] = lib or LIB   # (never what the caller's shell happens to name)
            f = os.path.join(outdir, f"{group}_{tag}.npz"); files.append(f)
            subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable, os.path.abspath(__file__), "child", group, f],
                           check=True, env=env)   # (the first non-zero exit ends the run)
        a, b = np.load(files[0]), np.load(files[1])
        assert a.files == b.files, group
        for k in a.files:
            arrays.append(k)
            if not (a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()):
                mismatches.append(k)
                print("DIFFERS", k, flush=True)
            if k.endswith("/status"):
                statuses[k[:-7]] = np.bincount(a[k], minlength=7).tolist()
        print(f"[ab] {group}: {len(a.files)} arrays, {len(mismatches)} mismatches so far", flush=True)
        a.close(); b.close()
        for f in files: os.remove(f)
    os.rmdir(outdir)
    with open(record, "w") as f:
        json.dump({"this": {"path": os.path.relpath(LIB, ROOT), "sha256": sha256(LIB)}, "other": {"path": os.path.basename(other), "sha256": sha256(other)},
                   "keys": KEYS, "arrays": arrays, "mismatches": mismatches, "status_counts": statuses}, f, indent=1)
    print(len(arrays), "arrays,", len(mismatches), "differ")
    raise SystemExit(1 if mismatches else 0)
