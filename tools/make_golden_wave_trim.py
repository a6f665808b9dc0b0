"""tests/golden/wave_trim.npz: the cases of tests/wave_trim_cases.py solved by the PARENT commit's libacn_qp_hip.so on the
GPU -- the bits that the wave kernel's EVSE extent, and any later change to its iteration, must keep.

    python tools/make_golden_wave_trim.py --check-twin          (CPU only: what the cases must exercise)
    python tools/make_golden_wave_trim.py <parent.so> [out.npz] (on the GPU)

--check-twin runs every case on the CPU twin (oracle/admm_port.c) and asserts that it holds a problem of >= 60
iterations (the ring of 5 slots, one event per 5 iterations, wraps: every slot written twice) and a problem that adapts
rho (the ring restarts): the twin does not report its adaptations, so a problem counts as adapting if its iteration count
changes when adaptation is switched off.  Recording runs the parent library in a child process of its own (ACNQP_LIBRARY
selects it, as in tools/gpu_bench_ab.py) under a time limit, and keeps x, status, iters, pri_res, dua_res, obj."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import wave_trim_cases as TC   # noqa: E402


def check_twin():
    from oracle import admm_port

    for name in TC.CASES:
        batch, skw = TC.build(name)
        kw = dict(threads=8, accel_mem=5)
        if skw.get("warm") == "self":
            first = admm_port.solve_batch(batch, **kw)
            kw.update(warm_x=first["x"] * np.random.default_rng(5).uniform(0.9, 1.0, size=first["x"].shape), warm_y=first["y"])
        a = admm_port.solve_batch(batch, **kw)
        b = admm_port.solve_batch(batch, adapt_every=0, **kw)
        adapts = np.flatnonzero(a["iters"] != b["iters"])
        print(f"{name}: B {batch.B} N {batch.site.N} T {batch.Tm} iters {a['iters'].min()}..{a['iters'].max()} "
              f"(>= 60: {(a['iters'] >= 60).sum()}), adapting rho: {adapts.size}, status {np.unique(a['status'])}", flush=True)
        assert (a["iters"] >= 60).any(), name
        assert adapts.size >= 1, name


if __name__ == "__main__":
    if sys.argv[1] == "--check-twin":
        check_twin()
        raise SystemExit(0)
    parent = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "wave_trim.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("ACNQP_WAVE_FULL_RANK", "ACNQP_WAVE_FULL_EVSE", "ACNQP_NO_WAVE", "ACNQP_NO_WAVE2", "ACNQP_WAVE_MIN_BATCH")}
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "parent.npz")
        subprocess.run(["timeout", "-k", "10", "300", sys.executable, TC.__file__, f, "--results-only"], check=True, env=dict(env, ACNQP_LIBRARY=parent))
        with np.load(f) as z:
            keep = {k: z[k] for k in z.files if k.split(":", 1)[1] in TC.KEYS}
    assert len(keep) == len(TC.CASES) * len(TC.KEYS)
    np.savez_compressed(out, **keep)
    print(out, os.path.getsize(out), "bytes;", {n: (int(keep[n + ':iters'].min()), int(keep[n + ':iters'].max())) for n in TC.CASES})
