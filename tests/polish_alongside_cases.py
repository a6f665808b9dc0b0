"""Cases for the polish launch that runs alongside the solver launch (acn_qp_polclaim.hpp).  Run as
a script it solves the named cases (default: all) under the environment it was started with -- ACNQP_NO_POLISH_ALONGSIDE=1:
the serial polish alone; ACNQP_POLISH_ALONGSIDE_SPINS=0: every workgroup alongside leaves without a look at the list -- and
saves the results, what acnqp_debug_polish_alongside reports after each case and the polish counters of the case.
tests/test_polish_alongside_gpu.py compares such runs with each other.

Every case is caltech54 with SOC rows and default_options(polish_iters=K), K a multiple of check_every chosen on the CPU
twin (oracle/admm_port.solve_batch, accel_mem=5) so that between a tenth and a half of the problems run past K: a large
share of a small batch is handed over, and the hand-overs arrive while other waves are still at work, not at the end.
Twin shares of problems with more than K iterations:
  lone_h12              horizon 12, 1,280 problems, K = 300: 0.249 -- solve_device; 1,024 wave slots: workgroups retire early
  one_per_wave          horizon 12,   256 problems, K = 300: 0.207 -- solve_device; nothing retires early
  pipelined_last_chunk  horizon 12, 9 x 256 problems, K = 300: 0.243 -- acnqp_solve_batches, several chunks
  h24_two_waves         horizon 24,   512 problems, K = 400: 0.342 -- solve_device; two waves per problem"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = ("lone_h12", "one_per_wave", "pipelined_last_chunk", "h24_two_waves")
SHAPE = {"lone_h12": (12, 1280, 300), "one_per_wave": (12, 256, 300), "pipelined_last_chunk": (12, 2304, 300), "h24_two_waves": (24, 512, 400)}   # horizon, problems, K
SEED = {"lone_h12": 9301, "one_per_wave": 9302, "pipelined_last_chunk": 9303, "h24_two_waves": 9305}
KEYS = ("x", "status", "iters", "pri_res", "dua_res", "obj")


def build(name):
    """The case's batches (one; nine of 256 for the pipelined case)."""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.builder import build_batch

    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    T, B, _ = SHAPE[name]
    if name == "pipelined_last_chunk":   # (the twin's share above: the nine batches together, seed 9303 as one batch of 2,304)
        return [build_batch(sites.snapshot_batch(infra, T, 256, seed=SEED[name] + 17 * g), infra, iface, obj, "SOC") for g in range(B // 256)]
    return [build_batch(sites.snapshot_batch(infra, T, B, seed=SEED[name]), infra, iface, obj, "SOC")]


def solve(name):
    import torch

    from adacharge_amd.backend import DeviceBatch, SiteHandle, default_options

    batches = build(name)
    opts = default_options(polish_iters=SHAPE[name][2])
    h = SiteHandle(batches[0].site, 0)
    h.polish_alongside()
    before = h.polish_stats()
    if len(batches) > 1:
        res = h.solve_many(batches, opts)
        out = {k: np.concatenate([getattr(r, k) for r in res]) for k in KEYS}
    else:
        dev = DeviceBatch(batches[0], "cuda:0")
        h.solve_device(dev, opts)
        torch.cuda.synchronize()
        out = {k: getattr(dev, k).cpu().numpy() for k in KEYS}
    out["alongside"] = h.polish_alongside()
    after = h.polish_stats()
    out["attempted"] = after["attempted"] - before["attempted"]
    out["solved"] = after["solved"] - before["solved"]
    out["family"] = h.route(batches[0].Tm, batches[0].K, batches[0].B)[0]
    h.close()
    return out


if __name__ == "__main__":
    flat = {}
    for name in (sys.argv[2:] or CASES):
        for k, v in solve(name).items():
            flat[f"{name}:{k}"] = v
    np.savez_compressed(sys.argv[1], **flat)
