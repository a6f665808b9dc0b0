"""Oracle-certified fixtures at the shape edges of every kernel route (tests/golden/edges.npz, generator
tools/make_golden_edges.py): each case sits on one side of a cut of the routing rule (N 64/65, horizons 12/13, 16/17,
24/25, 32/33, 48/49, 288/289, 16/32/48 padded site rows, four session slots per EVSE) and records the kernel family it
is written for -- ragged N (padded lanes, a partly padded last EVSE tile up to N = 1,023), dead period registers,
partial MFMA tiles.

CPU (`-m "not gpu"`): the stored optimum is feasible for the problem the builder states and its objective matches;
the C twin of the device algorithm reaches it.  GPU: the default surface against the certificate, the family
acnqp_route reports against the one the fixture declares, and the case's bits inside a 257-problem launch of its own
shape against the lone solve."""
import numpy as np
import pytest

from adacharge_amd import AdaptiveChargingOptimization
from adacharge_amd.builder import ProblemBatch, build_batch, scenario_batch
from tests import helpers as H

RATE_TOL = 1e-4 * 32.0   # north star: 1e-4 relative on rates, 32 A pilots
NAMES = [str(n) for n in H.load_edges()["names"]]
# the C twin (one CPU thread, tight tolerances) takes minutes on these: the GPU tests cover them
SLOW_ON_CPU = {"n4_t289", "n1023_t12_soc", "n64_t49_lin", "n65_t49_lin", "n65_t49_soc"}


def _case(name):
    return H.edges_case(H.load_edges(), name)


def _batch(name):
    sl, infra, iface, obj, meta, peak, exp = _case(name)
    return build_batch([sl], infra, iface, obj, meta["ct"], meta["eq"], peak_limits=[peak])


def _site_rows_ok(rates, infra, ct, tol):
    if ct == "SOC":
        H.assert_infrastructure_satisfied(rates, infra, tol=tol)
    else:
        assert (np.abs(infra.constraint_matrix) @ rates <= infra.constraint_limits[:, None] + tol).all()


def test_fixture_covers_every_family_and_both_cones():
    g = H.load_edges()
    fams = {str(g[f"{n}_family"]) for n in NAMES}
    assert fams == {"wave1", "wave2", "wave3", "wave4", "wave5", "tiled_ct1", "tiled_ct2", "long_lds", "long_ws",
                    "stream", "general"}, fams
    cones = {int(g[f"{n}_meta"][1]) for n in NAMES}
    assert cones == {0, 1}
    assert all(float(g[f"{n}_cert"].max()) <= 1e-9 for n in NAMES)
    # the ragged widths the kernels pad: N = 1, 17, 65, 79, 100, 1,023 (not multiples of 16)
    assert {1, 17, 65, 79, 100, 1023} <= {int(g[f"{n}_cm"].shape[1]) for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_feasible_for_the_builders_statement(name):
    sl, infra, iface, obj, meta, peak, exp = _case(name)
    batch = build_batch([sl], infra, iface, obj, meta["ct"], meta["eq"], peak_limits=[peak])
    r = exp["rates"]
    T = int(batch.T[0])
    assert T == meta["T"] == batch.Tm and r.shape == (infra.num_stations, T)
    assert (r >= batch.lb[0, :, :T] - 1e-7).all() and (r <= batch.ub[0, :, :T] + 1e-7).all()
    for k in range(batch.K):
        for i in range(batch.N):
            L = int(batch.s_len[0, k, i])
            if L:
                o = int(batch.s_off[0, k, i])
                e = r[i, o:o + L].sum()
                assert e <= batch.s_cap[0, k, i] + 1e-6
                if meta["eq"]:
                    assert abs(e - batch.s_cap[0, k, i]) <= 1e-6 * max(1.0, batch.s_cap[0, k, i])
    _site_rows_ok(r, infra, meta["ct"], 1e-6)
    if peak is not None:
        assert (r.sum(axis=0) <= np.broadcast_to(peak, (T,)) + 1e-6).all()
    full = 0.5 * batch.pdiag[0] * (r ** 2).sum() + (batch.q[0, :, :T] * r).sum()
    if batch.site.has_flat:
        full += 0.5 * batch.lf[0] * ((batch.site.G[batch.site.flat_row] @ r) ** 2).sum()
    if batch.site.has_max:
        full += batch.dc[0] * max(float((batch.site.G[batch.site.max_row] @ r).max()), float(batch.dfloor[0]))
    # (load_flattening's constant sum_t ext_t^2, aco.py:408, is left out on both sides: no solver sees it)
    assert abs(full - exp["obj"]) <= 1e-9 * abs(exp["obj"]), (full, exp["obj"])


@pytest.mark.parametrize("name", [n for n in NAMES if n not in SLOW_ON_CPU])
def test_c_twin_reaches_the_certified_optimum(name):
    from oracle import admm_port

    batch = _batch(name)
    exp = _case(name)[-1]
    out = admm_port.solve_batch(batch, eps_abs=1e-9, eps_rel=1e-9, max_iter=100000, accel_mem=5)
    assert out["status"][0] == 1, (name, out["status"], out["iters"])
    T = int(batch.T[0])
    d = float(np.abs(out["x"][0][:, :T] - exp["rates"]).max())
    assert d <= RATE_TOL, (name, d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_path_reaches_the_certified_optimum_on_its_route(name):
    from adacharge_amd.backend import SiteHandle

    sl, infra, iface, obj, meta, peak, exp = _case(name)
    opt = AdaptiveChargingOptimization(obj, iface, constraint_type=meta["ct"], enforce_energy_equality=meta["eq"])
    rates = opt.solve(sl, infra, peak_limit=peak)   # default options: the drop-in surface as a caller gets it
    assert int(opt.last_result.status[0]) == 1, (name, opt.last_result.status, opt.last_result.iters)
    d = float(np.abs(rates - exp["rates"]).max())
    assert d <= RATE_TOL, (name, meta, d)
    assert abs(float(opt.last_result.obj[0]) - exp["obj"]) <= 1e-6 * abs(exp["obj"]), (name, opt.last_result.obj[0], exp["obj"])
    _site_rows_ok(rates, infra, meta["ct"], 1e-3)   # the reference's invariant (t_aco.py:76-83)
    batch = opt.last_batch
    h = SiteHandle(batch.site, 0)
    family, _ = h.route(batch.Tm, batch.K, 1)
    h.close()
    assert family == meta["family"], (name, family, meta["family"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_inside_a_257_problem_launch(name):
    """The case as one problem of a launch of 257 at a random position; the other 256 are the same snapshot with its
    demands scaled by U(0.85, 1) -- same site, horizon and session slots, so the launch's t_max and K are the case's."""
    import torch
    from adacharge_amd.backend import DeviceBatch, SiteHandle

    base = _batch(name)
    rng = np.random.default_rng(int(_case(name)[4]["seed"]))
    filler = scenario_batch(base, rng.uniform(0.85, 1.0, size=(256, base.K, base.N)))
    pos = int(rng.integers(0, 257))
    big = ProblemBatch.concatenate([filler.subset(np.arange(pos)), base, filler.subset(np.arange(pos, 256))])
    assert big.B == 257 and big.Tm == base.Tm and big.K == base.K
    h = SiteHandle(base.site, 0)
    lone = h.solve(base)
    dev = DeviceBatch(big, "cuda:0")
    h.solve_device(dev, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h.close()
    assert int(dev.status[pos]) == int(lone.status[0]) == 1, (name, int(dev.status[pos]), int(lone.status[0]))
    assert int(dev.iters[pos]) == int(lone.iters[0]), (name, int(dev.iters[pos]), int(lone.iters[0]))
    assert np.array_equal(dev.x[pos].cpu().numpy(), lone.x[0]), name
