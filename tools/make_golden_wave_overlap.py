"""tests/golden/wave_overlap.npz: the cases of tests/wave_overlap_cases.py solved by the PARENT commit's libacn_qp_hip.so on
the GPU -- the bits that the placement of the wave kernel's vector work beside its matrix chains must keep (DESIGN.md
section 3.1, "overlap").

    python tools/make_golden_wave_overlap.py --check-twin          (CPU only: what the cases must exercise)
    python tools/make_golden_wave_overlap.py <parent.so> [out.npz] (on the GPU)

--check-twin solves the cases of LONG_AND_ADAPTING on the CPU twin (oracle/admm_port.c) and asserts that each holds a
problem of >= 60 iterations and a problem that adapts rho (its iteration count changes when adaptation is switched off:
the twin does not report its adaptations), and that the equality case's start point clips every period of every session
(the flat piece with an open bracket).  Recording runs the parent library in a child process of its own (ACNQP_LIBRARY
selects it, as in tools/gpu_bench_ab.py) under a time limit, and keeps x, status, iters, pri_res, dua_res, obj, and y
for the cases of WITH_Y."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import wave_overlap_cases as OC   # noqa: E402


def kept(name):
    return OC.KEYS + (("y",) if name in OC.WITH_Y else ())


def check_twin():
    from oracle import admm_port

    for name in OC.LONG_AND_ADAPTING:
        batch, okw, _ = OC.build(name)
        kw = dict(threads=8, accel_mem=5, **okw)
        a = admm_port.solve_batch(batch, **kw)
        b = admm_port.solve_batch(batch, adapt_every=0, **kw)
        adapts = np.flatnonzero(a["iters"] != b["iters"])
        print(f"{name}: B {batch.B} iters {a['iters'].tolist()}, adapting rho: {adapts.tolist()}, status {np.unique(a['status'])}", flush=True)
        assert (a["iters"] >= 60).any() and adapts.size >= 1, name
    batch, _, _ = OC.build("equality")
    assert batch.s_eq.all() and batch.K == 1
    start = -1e5 * batch.q   # (kStartGain, acn_qp_common.hpp)
    clipped = (start >= batch.ub) | (start <= batch.lb)
    live = batch.s_len[:, 0, :] > 0
    print(f"equality: {int(live.sum())} sessions, start point clipped in every period: {bool(clipped.all(axis=2)[live].all())}", flush=True)
    assert live.any() and clipped.all(axis=2)[live].all()


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] in ("-h", "--help"):
        raise SystemExit(__doc__)
    if sys.argv[1] == "--check-twin":
        check_twin()
        raise SystemExit(0)
    parent = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "wave_overlap.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("ACNQP_")}
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "parent.npz")
        subprocess.run(["timeout", "-k", "10", "300", sys.executable, OC.__file__, f], check=True, env=dict(env, ACNQP_LIBRARY=parent))
        with np.load(f) as z:
            keep = {k: z[k] for k in z.files if k.split(":", 1)[1] in kept(k.split(":", 1)[0])}
            families = {n: str(z[n + ":family"]) for n in OC.CASES}
    assert len(keep) == sum(len(kept(n)) for n in OC.CASES)
    np.savez_compressed(out, **keep)
    print(out, os.path.getsize(out), "bytes;", {n: (families[n], int(keep[n + ':iters'].min()), int(keep[n + ':iters'].max()), np.unique(keep[n + ':status']).tolist()) for n in OC.CASES})
