"""Batch-size invariance (DESIGN.md sections 2.3 and 3.1: a problem's result must not depend on what it is batched with).

The statement tested: problems of the SAME padded shape (t_max, k_sessions) on one site give the same bits -- schedule,
status and iteration count -- whatever the size of the launch that carries them and however a call is cut into
chunks.  A launch of another t_max or K legitimately runs another kernel family (include/acn_qp.h, ACNQP_ROUTE_*) and
is out of scope.

Pools rich in stragglers (problems that reach the polish hand-over at 800 ADMM iterations), 8 x CUs + 1 problems each,
so that the full launch is one problem past the largest launch a per-launch-size rule could still treat as "small":
  - BASELINE.json configs[3], site 3 (36 EVSE, two row tiles, horizon 12): demand scenarios of one snapshot,
    bench.py's cfg3_site generator restated here;
  - configs[2] snapshots, jpl52 x 24 (wave kernel, four waves) and caltech54 x 24 (wave kernel, two waves);
  - jpl52 x 28 (long-horizon kernel, LDS variant).
Each pool: the full launch, a launch of the 256 problems the full launch needed the most iterations for, and the
worst one alone (device entry: one launch each), plus the pool through acnqp_solve_batches cut as [1,000, rest]."""
import numpy as np
import pytest

from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.builder import build_batch, scenario_batch

QC_ES = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)]


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _cfg3_site3(n):
    """bench.py's other_workloads()["cfg3_site3_T12_b1024"] generator, with n scenarios instead of 1,024"""
    infra = sites.eight_sites()[3]
    iface = Interface({"infrastructure_info": infra, "period": 5})
    rng = np.random.default_rng(500 + 3)
    base = build_batch([sites.random_sessions(infra, 12, rng)], infra, iface, QC_ES, "SOC")
    return scenario_batch(base, rng.lognormal(0.0, 0.25, size=(n, base.K, base.N)))


def _snapshots(site_name, T, seed):
    def make(n):
        infra = getattr(sites, site_name)()
        iface = Interface({"infrastructure_info": infra, "period": 5})
        return build_batch(sites.snapshot_batch(infra, T, n, seed=seed), infra, iface, QC_ES, "SOC")
    return make


# name: (generator of n problems, kernel family, the pool has stragglers that reach the polish)
POOLS = {
    "cfg3_site3_T12": (_cfg3_site3, "wave3", True),
    "jpl52_T24": (_snapshots("jpl52", 24, 31), "wave4", True),
    # (no caltech54 x 24 snapshot of this generator runs past the polish hand-over: 0 of 2,049, and none of the harder
    #  snapshot or scenario generators tried either -- this pool pins the bits and the route only)
    "caltech54_T24": (_snapshots("caltech54", 24, 31), "wave2", False),
    "jpl52_T28": (_snapshots("jpl52", 28, 28), "long_lds", True),
}


def _launch(h, batch):
    """one launch through the device entry point (acnqp_solve_batch_device): (x, status, iters) on the host"""
    import torch
    from adacharge_amd.backend import DeviceBatch

    dev = DeviceBatch(batch, "cuda:0")
    h.solve_device(dev, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dev.x.cpu().numpy(), dev.status.cpu().numpy(), dev.iters.cpu().numpy()


def _same(name, what, idx, ref, got):
    """bitwise equality of (x, status, iters) of the shared problems; the message names the problems that differ"""
    xr, sr, ir = (a[idx] for a in ref)
    xg, sg, ig = got
    diff = np.flatnonzero((sr != sg) | (ir != ig) | np.any(xr != xg, axis=(1, 2)))
    assert diff.size == 0, (
        f"{name}: {what} differs from the full launch on {diff.size} of {len(idx)} problems; first ones "
        + ", ".join(f"#{int(idx[k])}: status {int(sr[k])} iters {int(ir[k])} (full) vs status {int(sg[k])} iters {int(ig[k])}"
                    for k in diff[:6]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_same_shape_same_bits_whatever_the_launch_size(name):
    from adacharge_amd.backend import SiteHandle, default_options

    make, family, stragglers = POOLS[name]
    big = 8 * _cus() + 1
    pool = make(big)
    assert pool.B == big
    h = SiteHandle(pool.site, 0)
    before = h.polish_stats()["attempted"]
    full = _launch(h, pool)
    after_full = h.polish_stats()["attempted"]
    worst = np.sort(np.argsort(full[2], kind="stable")[-256:])
    small = _launch(h, pool.subset(worst))
    after_small = h.polish_stats()["attempted"]
    one = int(worst[np.argmax(full[2][worst])])
    alone = _launch(h, pool.subset(np.array([one])))

    _same(name, "the 256-problem launch of its stragglers", worst, full, small)
    _same(name, "the worst problem alone", np.array([one]), full, alone)
    # the pools really cross the polish: the stragglers reach it in the small launch AND in the large one
    if stragglers:
        assert after_small > after_full, (name, before, after_full, after_small)
        assert after_full > before, (name, before, after_full, after_small)

    # the pipelined entry (acnqp_solve_batches, chunks on four streams) over the pool cut in two
    cut = 1000
    parts = h.solve_many([pool.subset(np.arange(cut)), pool.subset(np.arange(cut, big))], default_options())
    many = (np.concatenate([r.x for r in parts]), np.concatenate([r.status for r in parts]), np.concatenate([r.iters for r in parts]))
    _same(name, "solve_many [1000, rest]", np.arange(big), full, many)
    # the route is a function of the shape: same family and same polish decision for every launch size
    routes = {b: h.route(pool.Tm, pool.K, b) for b in (1, 256, big)}
    h.close()
    assert routes[1] == (family, True), routes
    assert routes[256] == routes[1] and routes[big] == routes[1], routes
